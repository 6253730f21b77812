"""GPU tests of the learner clock (``sgw_learn_clock``; sorrel_amd/csrc/learn_clock.h): each clocked call, with the clock at a value, leaves
the bits of its unclocked twin given that value as a scalar -- the draw of ``sgw_noisy_weights`` (both words), the turn of
``sgw_iqn_forward`` (the low word), the bound of ``sgw_sample``'s drawn starts (clamped in the kernel to ``[1, desc.num_starts]``) -- and
``sgw_learn_clock_advance`` adds one to the count and touches nothing else."""
import ctypes as C

import numpy as np
import pytest
import torch

from sorrel_amd import _native as N
from sorrel_amd.buffers import Buffer, _launch_sample, _ring_layout, _sample_outputs
from tests import iqn_learner_common as LC
from tests import learner_common as LK
from tests import noisy_common as NC

pytestmark = pytest.mark.gpu
DEV = LK.DEV
COUNTS = (0, 1, (1 << 32) - 1, 1 << 32, (1 << 32) + 5)          # the high word must count (noisy) and must not (forward)


def clock_of(count=0, num_starts=0, reserved=(0, 0)):
    return torch.tensor([count, num_starts, *reserved], dtype=torch.int64, device=DEV)


# ------------------------------------------------------------------------------------------------------------------ noisy
JOB_COUNTS = (0, 1, 5, 257, 1025, 3, 4, 255, 256, 0, 1024, 2049, 7, 1, 5, 257, 1025, 2)        # 18 jobs


def _upload(array):
    g = LK.Guarded(torch, max(array.size, 1), np.float32, shift=4)
    if array.size:
        g.buf[g.lo:g.lo + array.nbytes].copy_(torch.from_numpy(np.ascontiguousarray(array).view(np.uint8).reshape(-1)))
    return g


def _noisy_forward(inputs, seed, draw, clock):
    """One drawn forward call over ``inputs`` = [(weight, sigma) guarded]: the guarded (out_eff, out_eps) of every job."""
    outs, jobs = [], []
    for k, (gw, gs, count) in enumerate(inputs):
        go, gn = LK.Guarded(torch, max(count, 1), np.float32, shift=4), LK.Guarded(torch, max(count, 1), np.float32, shift=12)
        outs.append((go, gn))
        jobs.append(dict(weight=gw.ptr, sigma=gs.ptr, out_eff=go.ptr, out_eps=gn.ptr, count=count, tensor_id=k + 3))
    d = NC.desc(N.NOISY_FORWARD, jobs, seed=seed, draw=draw)
    N.launch("sgw_noisy_weights", d, torch.device(DEV), clock=None if clock is None else clock.data_ptr())
    torch.cuda.synchronize()
    return outs


def test_noisy_clocked_is_the_unclocked_call_at_draw_equal_count():
    rng = np.random.default_rng(7)
    inputs = []
    for count in JOB_COUNTS:
        w, s = rng.standard_normal(count).astype(np.float32), (rng.standard_normal(count) * 0.3).astype(np.float32)
        inputs.append((_upload(w), _upload(s), count))
    seed, seen = NC.BASE_KEY[0], []
    for c in COUNTS:
        clock = clock_of(c, 3, (11, 13))
        want = _noisy_forward(inputs, seed, c, None)
        got = _noisy_forward(inputs, seed, 0, clock)
        for k, (count, (go, gn), (wo, wn)) in enumerate(zip(JOB_COUNTS, got, want)):
            ctx = (c, k, count)
            assert go.intact() and gn.intact() and wo.intact() and wn.intact(), ctx
            LK.same_bits(go.numpy(), wo.numpy(), "out_eff", ctx)               # (the whole body: past count it is still 0xA5 on both sides)
            LK.same_bits(gn.numpy(), wn.numpy(), "out_eps", ctx)
        assert clock.tolist() == [c, 3, 11, 13]                                  # read only
        seen.append(np.concatenate([gn.numpy()[:count] for count, (_, gn) in zip(JOB_COUNTS, got)]))
    for a in range(len(COUNTS)):
        for b in range(a + 1, len(COUNTS)):                                      # 2^32 is not 0 and 2^32 + 5 is not 5: the high word counts
            assert (seen[a] != seen[b]).mean() > 0.9, (COUNTS[a], COUNTS[b])


def test_noisy_clocked_backward_gives_the_unclocked_bits():
    counts = (1025, 0, 5, 257, 1, 256)
    got = []
    for clock in (None, clock_of((1 << 32) + 5, 1)):
        outs, jobs = [], []
        r = np.random.default_rng(9)                              # the same inputs on both sides
        for count in counts:
            g, e = r.standard_normal(count).astype(np.float32), r.standard_normal(count).astype(np.float32)
            gg, ge, go = _upload(g), _upload(e), LK.Guarded(torch, max(count, 1), np.float32, shift=4)
            outs.append((go, g, e, gg, ge))
            jobs.append(dict(grad_eff=gg.ptr, eps_in=ge.ptr, out_grad_sigma=go.ptr, count=count))
        N.launch("sgw_noisy_weights", NC.desc(N.NOISY_BACKWARD, jobs), torch.device(DEV), clock=None if clock is None else clock.data_ptr())
        torch.cuda.synchronize()
        got.append(outs)
    for count, (go, g, e, gg, ge), (wo, *_rest) in zip(counts, got[1], got[0]):
        assert go.intact() and gg.intact() and ge.intact(), count
        LK.same_bits(go.numpy(), wo.numpy(), "out_grad_sigma", count)
        LK.same_bits(go.numpy()[:count], g * e, "out_grad_sigma", count)


# ------------------------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("rows", (1, 6, 65))
@pytest.mark.parametrize("shape", LC.SHAPES, ids=LC.tag_of)
def test_forward_clocked_is_the_unclocked_call_at_turn_equal_the_low_word(shape, rows):
    from sorrel_amd.models.iqn import IQN

    obs, n_frames, L, Nq, A, _ = shape
    net = IQN((obs,), A, L, LC.SEED, Nq, n_frames, device=torch.device(DEV))
    x = torch.randn((rows, obs * n_frames), generator=torch.Generator().manual_seed(rows)).to(DEV)
    ws = net.weight_list()
    taus_of = {}
    for epoch in (0, 2):
        for c in COUNTS:
            clock = clock_of(c, 1, (5, 6))
            key = {"seed": 0x1234567887654321, "epoch": epoch, "num_envs": rows, "first_env": 3}
            _, flat, _, want = net._check_call(x, Nq, None, None)
            net._launch_forward(flat, ws, want, None, dict(key, turn=c & 0xFFFFFFFF))
            _, flat, _, got = net._check_call(x, Nq, None, None)
            got.taus.fill_(-1.0)
            net._launch_forward(flat, ws, got, None, dict(key, turn=0, clock=clock.data_ptr()))
            torch.cuda.synchronize()
            ctx = (shape, rows, epoch, c)
            LK.same_bits(got.taus.cpu().numpy(), want.taus.cpu().numpy(), "out_taus", ctx)
            LK.same_bits(got.quantiles.cpu().numpy(), want.quantiles.cpu().numpy(), "out_quantiles", ctx)
            LK.same_bits(got.qvalues.cpu().numpy(), want.qvalues.cpu().numpy(), "out_qvalues", ctx)
            assert clock.tolist() == [c, 1, 5, 6]
            taus_of[(epoch, c)] = got.taus.cpu().numpy().copy()
    for epoch in (0, 2):
        assert np.array_equal(taus_of[(epoch, 1 << 32)], taus_of[(epoch, 0)])                      # the turn is 32 bits wide
        assert not np.array_equal(taus_of[(epoch, 1)], taus_of[(epoch, 0)])
        assert not np.array_equal(taus_of[(epoch, (1 << 32) + 5)], taus_of[(epoch, 0)])
    assert not np.array_equal(taus_of[(0, 1)], taus_of[(2, 1)])                                     # the epoch is the descriptor's
    # 2^32 + 5 is turn 5
    _, flat, _, five = net._check_call(x, Nq, None, None)
    net._launch_forward(flat, ws, five, None, {"seed": 0x1234567887654321, "epoch": 2, "num_envs": rows, "first_env": 3, "turn": 5})
    assert np.array_equal(five.taus.cpu().numpy(), taus_of[(2, (1 << 32) + 5)])


# ------------------------------------------------------------------------------------------------------------------ sample
@pytest.mark.parametrize("n_frames", (1, 5))
def test_sample_clocked_draws_below_the_clamped_bound(n_frames):
    capacity, E, obs, B = 16, 3, 7, 37
    g = torch.Generator().manual_seed(n_frames)
    ring = Buffer(capacity=capacity, obs_shape=(obs,), n_frames=n_frames, num_envs=E, device=torch.device(DEV))
    for _ in range(capacity):
        ring.add(torch.randn((E, obs), generator=g).to(DEV), torch.randint(0, 4, (E,), generator=g).to(DEV), torch.randn((E,), generator=g).to(DEV),
                 (torch.rand((E,), generator=g) < 0.2).float().to(DEV))
    layout = _ring_layout(ring, None)
    bound = capacity - n_frames                                   # the largest bound the host accepts: the last row read is the ring's last
    seen = set()
    for call, value in enumerate((1, 3, bound, bound + 100, 0, -7)):
        clamped = min(max(value, 1), bound)
        results = []
        for clock in (None, clock_of(99, value, (1, 2))):
            outs = _sample_outputs(B, n_frames, layout["R"], torch.device(DEV))
            for t in outs:
                t.fill_(-3)
            index = torch.full((B, 2), -1, dtype=torch.int64, device=DEV)
            count = torch.tensor([call + 5], dtype=torch.int64, device=DEV)
            _launch_sample(layout, n_frames, B, outs, index, None, None, clamped if clock is None else bound, count=count, seed=41,
                           clock=None if clock is None else clock.data_ptr())
            torch.cuda.synchronize()
            assert int(count) == call + 6                         # the device counter advanced by one
            results.append((index.cpu().numpy(), [t.cpu().numpy() for t in outs]))
            if clock is not None:
                assert clock.tolist() == [99, value, 1, 2]
        (want_index, want), (got_index, got) = results
        ctx = (n_frames, value)
        LK.same_bits(got_index, want_index, "out_index", ctx)
        for k, (a, b) in enumerate(zip(got, want)):
            LK.same_bits(a, b, f"output {k}", ctx)
        assert got_index[:, 0].min() >= 0 and got_index[:, 0].max() < clamped, ctx      # no start reaches the clamped bound
        assert got_index[:, 1].min() >= 0 and got_index[:, 1].max() < E, ctx
        seen.add(int(got_index[:, 0].max()))
    assert max(seen) >= 3                                          # (the larger bounds were used)


# ------------------------------------------------------------------------------------------------------------------ advance
def test_advance_adds_one_across_the_low_word_and_touches_nothing_else():
    clock = clock_of((1 << 32) - 2, -7, (0x0123456789ABCDEF, -1))
    lib = N.load()
    for _ in range(3):
        N.call(0, lib.sgw_learn_clock_advance, clock.data_ptr(), N.raw_stream(0))
    torch.cuda.synchronize()
    assert clock.tolist() == [(1 << 32) + 1, -7, 0x0123456789ABCDEF, -1]
    assert C.sizeof(N.SgwLearnClock) == clock.numel() * 8
