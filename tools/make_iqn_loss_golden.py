"""TEST INFRASTRUCTURE ONLY -- generate ``tests/golden/iqn_loss/quantile_huber.npz`` from the reference's IQN learner.

Needs the reference checkout (``oracle/ref_loader.py``).  Usage::

    PYTHONDONTWRITEBYTECODE=1 python tools/make_iqn_loss_golden.py

What runs is the reference's own ``iRainbowModel.train_step`` (``sorrel/models/pytorch/iqn.py``) on hand-filled ``Buffer``s with
``n_frames = 2`` and ``dones`` placed so that ``valid`` is 0 for some rows, once per set.  Nothing of it is restated:
``model.memory.sample`` is wrapped to keep the batch; ``qnetwork_local`` and ``qnetwork_target`` are replaced by small modules that return
prescribed ``[B, N, A]`` tensors and taus and call ``retain_grad()`` on their output, so that after the call's one ``backward`` the
``.grad`` of the third output is the gradient of the loss at ``q_expected`` (and that of the first stays absent: nothing flows through
the action choice); ``iqn.calculate_huber_loss`` is wrapped for the duration of the call to keep ``td_error``.  Stored per set: the
inputs, ``td_error``, the returned loss, the gradient at ``q_expected`` and the (zero) gradient at the first local call.  Data only.

One set is hand-made: every value is dyadic and small, so that every order of every sum gives the same bits; it holds exact
``td == 0``, exact ``|td| == 1`` and exactly tied action means.

The generator asserts, on the CPU, what makes the comparisons mean something (``tests/iqn_loss_common.py`` holds the formulas): every
Huber branch and both signs of ``td``, both ``valid`` values and both ``dones`` values occur in every set with B >= 32; outside the
hand-made set the two largest action means differ by more than ``N 2^-24`` times the sum of the magnitudes (torch's reduction order
cannot move an argmax) and no ``|td|`` lies within a relative ``2^-20`` of 1; ``next_actions``, ``td_error`` and the gradient's zeros
equal the restatement's bit for bit; and the reference's own gradient and loss lie within HALF of each tolerance formula of the
restatement.  It prints the share the reference uses."""
from __future__ import annotations

import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import ref_loader  # noqa: E402
from tests import iqn_loss_common as LC  # noqa: E402

OUT = LC.FIXTURE
OBS, N_FRAMES, N_STEP, GAMMA = 3, 2, 3, 0.99
# (action_space, n_quantiles, batch_size)
SETS = ((2, 1, 2), (3, 2, 37), (4, 12, 64), (5, 8, 37), (9, 13, 37), (17, 64, 2), (4, 64, 1))
HAND = (3, 4, 32)             # the hand-made set, with GAMMA = 0.5 and n_step = 2: a discount of exactly 0.25; B N N = 512 is dyadic too


def prescribed(rng, A, N, B, handmade):
    f32 = np.float32
    if handmade:
        qe = rng.integers(-12, 13, size=(B, N, A)).astype(f32) / f32(8)
        ql = rng.integers(-2, 3, size=(B, N, A)).astype(f32) / f32(4)
        qt = rng.integers(-8, 9, size=(B, N, A)).astype(f32) / f32(2)
        taus = rng.integers(1, 8, size=(B, N, 1)).astype(f32) / f32(8)
    else:
        qe = rng.normal(0.0, 1.5, size=(B, N, A)).astype(f32)
        ql = rng.normal(0.0, 1.5, size=(B, N, A)).astype(f32)
        qt = rng.normal(0.0, 1.5, size=(B, N, A)).astype(f32)
        taus = rng.random(size=(B, N, 1)).astype(f32)
    return qe, ql, qt, taus


def run_reference(iqn, torch, A, N, B, seed, handmade):
    gamma, n_step = (0.5, 2) if handmade else (GAMMA, N_STEP)
    cap = B + N_FRAMES + 2
    model = iqn.iRainbowModel(input_size=(OBS,), action_space=A, layer_size=4, epsilon=0.0, device="cpu", seed=seed, n_frames=N_FRAMES,
                              n_step=n_step, batch_size=B, memory_size=cap, GAMMA=gamma, n_quantiles=N)
    rng = np.random.default_rng(seed)
    mem = model.memory
    assert mem.n_frames == N_FRAMES >= 2
    mem.states[:] = rng.normal(size=mem.states.shape).astype(np.float32)
    mem.actions[:] = rng.integers(0, A, size=cap)
    mem.rewards[:] = (rng.integers(-4, 5, size=cap).astype(np.float32) * np.float32(0.5 if handmade else 0.37)).astype(np.float32)
    mem.dones[:] = (rng.random(size=cap) < 0.3).astype(np.float32)
    mem.idx, mem.size = 0, cap
    qe, ql, qt, taus = prescribed(rng, A, N, B, handmade)
    seen = {"outputs": []}

    class Prescribed(torch.nn.Module):
        def __init__(self, tables, taus_):
            super().__init__()
            self.tables = torch.nn.ParameterList([torch.nn.Parameter(torch.tensor(t)) for t in tables])
            self.taus_, self.calls = torch.tensor(taus_), 0

        def forward(self, states, n_quantiles):
            assert n_quantiles == N and states.shape == (B, OBS * N_FRAMES)
            out = self.tables[self.calls] * 1.0
            self.calls += 1
            out.retain_grad()
            seen["outputs"].append(out)
            return out, self.taus_

    model.qnetwork_local, model.qnetwork_target = Prescribed([ql, qe], taus), Prescribed([qt], taus)
    real_sample, real_huber = mem.sample, iqn.calculate_huber_loss

    def sample(batch_size):
        seen["batch"] = real_sample(batch_size=batch_size)
        return seen["batch"]

    def huber(td_errors, k=1.0):
        assert k == 1.0
        seen["td_error"] = td_errors.detach().clone()
        return real_huber(td_errors, k)

    mem.sample, iqn.calculate_huber_loss = sample, huber
    np.random.seed(seed)
    try:
        loss = model.train_step()
    finally:
        del mem.sample
        iqn.calculate_huber_loss = real_huber
    _states, actions, rewards, _next, dones, valid = seen["batch"]
    first_local, target_out, expected = seen["outputs"]
    assert model.qnetwork_local.calls == 2 and model.qnetwork_target.calls == 1
    assert first_local.grad is None                                        # nothing flows through the action choice
    del target_out       # (the reference does not detach the target net's output; its parameters are in no optimiser, and sgw_iqn_loss hands nothing on)
    assert actions.dtype == np.int64 and rewards.dtype == dones.dtype == np.float32 and valid.dtype == np.float64
    assert actions.shape == rewards.shape == dones.shape == valid.shape == (B, 1)
    td = seen["td_error"]
    assert td.dtype == torch.float32 and tuple(td.shape) == (B, N, N)
    return dict(q_expected=qe, taus=taus, q_next_local=ql, q_next_target=qt, actions=actions.copy(), rewards=rewards.copy(), dones=dones.copy(),
                valid=valid.copy(), discount=gamma ** n_step, td_error=td.numpy().copy(), loss=np.float64(loss),
                grad_expected=expected.grad.numpy().copy(), grad_next_local=np.zeros_like(ql))


def main() -> None:
    ref_loader.install()
    import torch
    from sorrel.models.pytorch import iqn

    arrays, meta = {}, dict(sets=[])
    runs = [(A, N, B, False) for A, N, B in SETS] + [HAND + (True,)]
    for i, (A, N, B, handmade) in enumerate(runs):
        tag = f"{'hand' if handmade else A}_{N}_{B}"
        s = run_reference(iqn, torch, A, N, B, 31 + i, handmade)
        info = LC.restate(*LC.inputs_of(s))
        assert not info["bad"].any()
        td, mag = info["td_error"], np.abs(info["td_error"])
        if B >= 32:
            assert (mag <= 1).any() and (mag > 1).any() and (td < 0).any() and (td > 0).any(), f"{tag}: a Huber branch or a sign does not occur"
            assert set(np.unique(s["valid"])) == {0.0, 1.0} and set(np.unique(s["dones"])) == {0.0, 1.0}, f"{tag}: valid or dones is constant"
        if handmade:
            assert (td == 0).any() and (mag == 1).any(), f"{tag}: no exact td == 0 or |td| == 1"
            top = np.sort(info["means"], axis=1)
            assert (top[:, -1] == top[:, -2]).any(), f"{tag}: no tied action means"
        else:
            if A > 1:
                top = np.sort(info["means"].astype(np.float64), axis=1)
                room = N * 2.0 ** -24 * np.abs(s["q_next_local"].astype(np.float64)).sum(axis=1).max(axis=1)
                assert ((top[:, -1] - top[:, -2]) > room).all(), f"{tag}: two action means lie within the reduction's rounding"
            assert (np.abs(mag.astype(np.float64) - 1.0) > 2.0 ** -20).all(), f"{tag}: a |td| lies at the Huber threshold"
        LC.same_bits(info["td_error"], s["td_error"], "td_error", tag)
        zeros = np.ones(s["grad_expected"].shape, bool)
        zeros[np.arange(B), :, s["actions"].reshape(B)] = False
        LC.same_bits(s["grad_expected"][zeros], np.zeros(int(zeros.sum()), np.float32), "the gradient's zeros", tag)
        tol = LC.tolerances(info)
        got = s["grad_expected"][np.arange(B), :, s["actions"].reshape(B)].astype(np.float64)
        share = dict(grad=float(np.max(np.abs(got - info["grad_at_action"].astype(np.float64)) / np.maximum(tol["grad"], 1e-300))),
                     L=float(abs(s["loss"] - info["L"]) / max(tol["L"], 1e-300)))
        if handmade:
            assert np.array_equal(info["grad"], s["grad_expected"]), f"{tag}: the gradient differs"      # (equal as numbers: a zero's sign is free)
            assert info["L"] == float(s["loss"])
        assert max(share.values()) <= 0.5, f"{tag}: the reference itself uses {share} of the tolerances"
        print(f"{tag}: discount {s['discount']!r}; |td| <= 1 in {float((mag <= 1).mean()):.2f} of the pairs; valid 0 in {int((s['valid'] == 0).sum())} rows; "
              f"share of the tolerance the reference uses: gradient {share['grad']:.4f} loss {share['L']:.4f}")
        for k in ("q_expected", "taus", "q_next_local", "q_next_target", "actions", "rewards", "dones", "valid", "td_error", "loss", "grad_expected",
                  "grad_next_local"):
            arrays[f"{k}_{tag}"] = s[k]
        meta["sets"].append(dict(tag=tag, A=A, N=N, B=B, discount=s["discount"], exact=handmade, next_local_grad_absent=True, share=share))
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, params=json.dumps(meta), **arrays)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
