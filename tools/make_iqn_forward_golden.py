"""TEST INFRASTRUCTURE ONLY -- generate ``tests/golden/iqn_forward/forward.npz`` from the reference's IQN network.

Needs the reference checkout (``oracle/ref_loader.py``).  Usage::

    PYTHONDONTWRITEBYTECODE=1 python tools/make_iqn_forward_golden.py

What runs is the reference's own ``IQN`` (``sorrel/models/pytorch/iqn.py``) on the CPU, per set once in eval mode on float32 states, once
in eval mode on uint8 one-hot states (widened by ``.float()``, as a learner does with a ``TurnBuffer``'s rows) and once in train mode.
Nothing of it is restated: ``calc_cos`` is wrapped to keep ``cos`` and ``taus``; a forward hook on each ``NoisyLinear`` keeps the
effective weights (``weight + sigma * epsilon`` of the buffers the call just filled).  The same forward is then evaluated in float64 (a
``.double()`` copy of the network whose ``calc_cos`` hands back the kept values).  Stored per set: the ``state_dict`` (after the train-mode
call, so its epsilon buffers are the noise that call used: the effective weights are recomposed from it, and asserted equal here), the inputs, and per mode taus, cos, the quantiles, their means over the
quantiles (what ``get_qvalues`` returns) and the float64 quantiles.  Data only.  In the reference's own shape the two large weight
matrices are set to multiples of a power of two before the run and stored as int8 (the file stays under the size limit).

The generator asserts, on the CPU, what makes the comparisons mean something (``tests/iqn_forward_common.py`` holds the formulas): the
restatement, fed the reference's own cos, lies within HALF of ``2 E`` of the reference (it prints the share used); on every set the two
largest qvalues of every row differ by more than ``4 E``, so the greedy action must equal the reference's; the effective weights the
hooks kept are ``weight + sigma * epsilon`` in float32 bit for bit.  It also prints the reference's ``cos`` against float64 ``cos`` of the
same float32 argument, in units of ``2^-24``."""
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
from tests import iqn_forward_common as FC  # noqa: E402

OUT = FC.FIXTURE
PACK = {"head1.weight": 11, "ff_1.weight": 10}          # the reference's own shape: value = int8 code * 2^-exponent


def run(iqn_mod, layers_mod, torch, net, states, N, train):
    seen = {}
    real = net.calc_cos

    def calc_cos(batch_size, n_tau=8):
        cos, taus = real(batch_size, n_tau)
        seen["cos"], seen["taus"] = cos.detach().clone(), taus.detach().clone()
        return cos, taus

    hooks = []
    for name in ("ff_1", "advantage", "value"):
        layer = getattr(net, name)
        assert isinstance(layer, layers_mod.NoisyLinear)

        def hook(mod, _inp, _out, name=name):
            if mod.training:
                seen[name] = ((mod.weight + mod.sigma_weight * mod.epsilon_weight).detach().clone(), (mod.bias + mod.sigma_bias * mod.epsilon_bias).detach().clone())
            else:
                seen[name] = (mod.weight.detach().clone(), mod.bias.detach().clone())

        hooks.append(layer.register_forward_hook(hook))
    net.train(train)
    net.calc_cos = calc_cos
    try:
        with torch.no_grad():
            quant, taus = net(states, N)
    finally:
        del net.calc_cos
        for h in hooks:
            h.remove()
    assert torch.equal(taus, seen["taus"])
    # float64: the same network, the same taus and cos
    net64 = copy.deepcopy(net).double()
    net64.train(False)
    if train:
        for name in ("ff_1", "advantage", "value"):
            layer = getattr(net64, name)
            layer.weight.data, layer.bias.data = seen[name][0].double(), seen[name][1].double()
    net64.calc_cos = lambda batch_size, n_tau=8: (seen["cos"].double(), seen["taus"].double())
    with torch.no_grad():
        quant64, _ = net64(states.double(), N)
    return dict(taus=seen["taus"].numpy().copy(), cos=seen["cos"].numpy().copy(), quantiles=quant.numpy().copy(), qvalues=quant.mean(dim=1).numpy().copy(),
                quantiles64=quant64.numpy().copy(), kept={k: (v[0].numpy().copy(), v[1].numpy().copy()) for k, v in seen.items() if k not in ("cos", "taus")})


def main() -> None:
    ref_loader.install()
    import torch
    from sorrel.models.pytorch import iqn, layers

    torch.set_num_threads(1)
    arrays, meta = {}, dict(sets=[])
    worst_cos = 0.0
    for i, (D, L, N, A, B) in enumerate(FC.SETS):
        tag = f"{D}_{L}_{N}_{A}_{B}"
        net = iqn.IQN((D,), A, L, seed=41 + i, n_quantiles=N, n_frames=1, device="cpu")
        rng = np.random.default_rng(41 + i)
        packed = {}
        if D * L > 65536:
            with torch.no_grad():
                for name, exp in PACK.items():
                    mod, attr = name.split(".")
                    t = getattr(getattr(net, mod), attr)
                    code = torch.round(t * 2.0 ** exp).clamp(-127, 127)
                    t.copy_(code * 2.0 ** -exp)
                    packed[name] = exp
                # the a-priori bound of this shape (K = 875 and 250) is wider than the gaps between action values that the initial
                # weights give: spread the advantage biases so that every row's greedy action is decided by more than 4 E
                net.advantage.bias.copy_(torch.tensor([0.0, 0.8, -0.8, 1.6][:A]))
        states = rng.normal(0.0, 1.0, size=(B, D)).astype(np.float32)
        states_u8 = (rng.random(size=(B, D)) < 0.15).astype(np.uint8)
        modes = {}
        modes["eval"] = run(iqn, layers, torch, net, torch.from_numpy(states), N, False)
        modes["u8"] = run(iqn, layers, torch, net, torch.from_numpy(states_u8).float(), N, False)
        modes["train"] = run(iqn, layers, torch, net, torch.from_numpy(states), N, True)
        sd = {k: v.numpy().copy() for k, v in net.state_dict().items()}
        shares = {}
        for mode, r in modes.items():
            x = states_u8 if mode == "u8" else states
            w = FC.effective_of(sd, mode == "train")
            for name, key in (("ff_1", "ff"), ("advantage", "adv"), ("value", "val")):
                FC.same_bits(r["kept"][name][0].reshape(w[f"w_{key}"].shape), w[f"w_{key}"], f"effective {name}.weight", tag + mode)
                FC.same_bits(r["kept"][name][1], w[f"b_{key}"], f"effective {name}.bias", tag + mode)
            quant, qv = FC.restate(w, x, r["cos"])
            q64, qv64, eq, eqv = FC.bound(w, x, r["cos"])
            assert np.abs(q64 - r["quantiles64"]).max() <= 1e-9 * (1 + np.abs(q64).max()), f"{tag} {mode}: the float64 forwards differ"
            share = max(float((np.abs(quant.astype(np.float64) - r["quantiles"]) / (2 * eq)).max()),
                        float((np.abs(qv.astype(np.float64) - r["qvalues"]) / (2 * eqv)).max()))
            own = max(float((np.abs(r["quantiles"] - q64) / eq).max()), float((np.abs(quant - q64) / eq).max()))
            assert share <= 0.5, f"{tag} {mode}: the restatement and the reference differ by {share} of 2 E"
            assert own <= 1.0, f"{tag} {mode}: a side lies {own} E from the exact value"
            if A > 1:
                top = np.sort(qv64, axis=1)
                assert ((top[:, -1] - top[:, -2]) > 4 * eqv.max(axis=1)).all(), f"{tag} {mode}: two qvalues lie within 4 E"
            args = FC.cos_args(r["taus"])
            assert np.array_equal(args, (r["taus"] * FC.pis()[None, None, :]).astype(np.float32))
            cerr = float((np.abs(r["cos"].astype(np.float64) - np.cos(args.astype(np.float64))) / FC.U).max())
            worst_cos = max(worst_cos, cerr)
            shares[mode] = share
            print(f"{tag} {mode}: share of 2 E between the restatement and the reference {share:.4f}; either side against float64 {own:.4f} E; "
                  f"max E quantiles {eq.max():.3g}, qvalues {eqv.max():.3g}; reference cos against float64 cos {cerr:.3f} x 2^-24")
            for k in ("taus", "cos", "quantiles", "qvalues", "quantiles64"):
                arrays[f"{tag}/{mode}/{k}"] = r[k]
        for k, v in sd.items():
            if k in packed:
                code = np.round(v.astype(np.float64) * 2.0 ** packed[k])
                assert np.array_equal((code * 2.0 ** -packed[k]).astype(np.float32), v)
                v = code.astype(np.int8)
            arrays[f"{tag}/sd/{k}"] = v
        arrays[f"{tag}/states"], arrays[f"{tag}/states_u8"] = states, states_u8
        meta["sets"].append(dict(tag=tag, D=D, L=L, N=N, A=A, B=B, sd_keys=sorted(sd), packed=packed, share=shares))
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, params=json.dumps(meta), **arrays)
    print(f"the reference's cos: at most {worst_cos:.3f} x 2^-24 from float64 cos of the same float32 argument")
    print(f"{OUT}: {os.path.getsize(OUT)} bytes")
    assert os.path.getsize(OUT) < (1 << 20)


if __name__ == "__main__":
    main()
