"""``sgw_sample`` on the device: the reference's own batch (``tests/golden/replay``) through the C ABI and through ``Buffer.sample``, a
grid of row lengths / stack depths / env counts / batch sizes against a numpy restatement of the reference's stacking, the
``TurnBuffer`` layouts, the grid-stride loop, indices out of range, indices drawn on the device (eagerly and in a replayed graph),
and the bytes around every output.  Every comparison is exact; no expectation comes from the kernel."""
import ctypes as C

import numpy as np
import pytest

from oracle import gridstep_oracle as O
from sorrel_amd import _native as N
from tests import sample_common as SC
from tests.gpu_common import torch_cuda  # noqa: F401
from tests.learner_common import DEV, Guarded

pytestmark = pytest.mark.gpu

def abi_sample(torch, states, actions, rewards, dones, n_frames, starts=None, envs=None, *, cols=None, num_starts=None, strides=None,
               offsets=(0, 0), R=None, offset_states=0, seed=0, draw=0, count=None, n=None):
    """One ``sgw_sample`` call over device rings ``[capacity, N, R]`` / ``[capacity, N]`` (or, with ``strides`` / ``offsets`` / ``cols``,
    whatever layout the caller describes); every output sits inside guards, which must come back untouched.  Returns the six arrays
    in the reference's order, the index array, and the raw output objects."""
    cap = int(states.shape[0])
    cols = int(states.shape[1]) if cols is None else cols
    R = int(np.prod(states.shape[2:])) if R is None else R
    n = len(starts) if starts is not None else n
    outs = dict(states=Guarded(torch, (n, n_frames * R), np.float32, offset_states), next_states=Guarded(torch, (n, n_frames * R), np.float32),
                actions=Guarded(torch, (n, 1), np.int64), rewards=Guarded(torch, (n, 1), np.float32),
                dones=Guarded(torch, (n, 1), np.float32), valid=Guarded(torch, (n, 1), np.float32), index=Guarded(torch, (n, 2), np.int64))
    d = N.SgwSampleDesc()
    d.states = states.data_ptr() + offsets[0] * states.element_size()
    d.actions = actions.data_ptr() + offsets[1] * actions.element_size()
    d.rewards, d.dones = rewards.data_ptr() + offsets[1] * 4, dones.data_ptr() + offsets[1] * 4
    keep = []
    if starts is not None:
        keep = [torch.as_tensor(np.asarray(starts, np.int64)).to(DEV), torch.as_tensor(np.asarray(envs, np.int64)).to(DEV)]
        d.starts, d.envs = keep[0].data_ptr(), keep[1].data_ptr()
    if count is not None:
        d.draw_count = count.data_ptr()
    d.out_states, d.out_next_states, d.out_actions = outs["states"].ptr, outs["next_states"].ptr, outs["actions"].ptr
    d.out_rewards, d.out_dones, d.out_valid, d.out_index = outs["rewards"].ptr, outs["dones"].ptr, outs["valid"].ptr, outs["index"].ptr
    d.n, d.capacity, d.num_envs, d.row_elems = n, cap, cols, R
    d.num_starts = cap - n_frames - 1 if num_starts is None else num_starts
    (d.state_turn_stride, d.state_env_stride), (d.scalar_turn_stride, d.scalar_env_stride) = strides or ((cols * R, R), (cols, 1))
    d.seed, d.draw = seed, draw
    d.n_frames = n_frames
    d.src_type = N.SAMPLE_U8 if states.dtype == torch.uint8 else N.SAMPLE_F32
    d.act_type = N.SAMPLE_ACT_U8 if actions.dtype == torch.uint8 else N.SAMPLE_ACT_I64
    N.check(N.load().sgw_sample(C.byref(d), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    for name, g in outs.items():
        assert g.intact(), f"bytes around out_{name} were written"
    six = tuple(outs[k].numpy() for k in SC.NAMES)
    return six, outs["index"].numpy(), outs


def f32_ring(rng, cap, E, R):
    """Host arrays of a Buffer-shaped ring: small-integer rows, dones on about a seventh of the slots."""
    states = rng.integers(-50, 50, size=(cap, E, R)).astype(np.float32)
    actions = rng.integers(0, 1 << 40, size=(cap, E)).astype(np.int64)
    rewards = rng.integers(-9, 10, size=(cap, E)).astype(np.float32)
    dones = (rng.random((cap, E)) < 0.15).astype(np.float32)
    return states, actions, rewards, dones


def up(torch, arrays):
    return tuple(torch.from_numpy(a).to(DEV) for a in arrays)


def indices(rng, n, num_starts, E):
    starts, envs = rng.integers(0, num_starts, size=n), rng.integers(0, E, size=n)
    starts[0], envs[0] = 0, E - 1
    if n > 2:
        starts[1], envs[1] = num_starts - 1, 0
        starts[2], envs[2] = starts[1], envs[1]              # a repeat
    return starts.astype(np.int64), envs.astype(np.int64)


# ------------------------------------------------------------------------------------------------------------- the reference's batch
def test_reference_batch_through_the_abi_and_buffer_sample(torch_cuda):
    torch = torch_cuda
    d = SC.load_fixture()
    buf = SC.replay_fixture(d, DEV)
    draws, zeros = d["draws"], np.zeros(len(d["draws"]), np.int64)
    six, index, _ = abi_sample(torch, buf.states, buf.actions, buf.rewards, buf.dones, buf.n_frames, draws, zeros,
                               num_starts=max(1, buf.size - buf.n_frames - 1))
    SC.assert_six(six, d["expected"], "sgw_sample")
    assert np.array_equal(index, np.stack([draws, zeros], axis=1))
    SC.assert_six(buf.sample(len(draws), starts=draws, envs=zeros), d["expected"], "Buffer.sample on the device")


# ------------------------------------------------------------------------------------------------------------- shapes
@pytest.mark.parametrize("E", [1, 3, 64])
@pytest.mark.parametrize("n_frames", [1, 2, 4])
@pytest.mark.parametrize("R", [1, 36, 75, 405])
def test_shapes_against_numpy(torch_cuda, R, n_frames, E):
    """n in {1, 3, 257} for every (row length, stack depth, env count); R = 36 also with out_states 4 bytes off (the dword variant)."""
    torch = torch_cuda
    cap = 24
    rng = np.random.default_rng(1000 * R + 10 * n_frames + E)
    host = f32_ring(rng, cap, E, R)
    num_starts = cap - n_frames - 1
    dev = up(torch, host)
    for n in (1, 3, 257):
        starts, envs = indices(rng, n, num_starts, E)
        if n_frames > 1:                                           # a done on a frame before the last (valid = 0) ...
            host[3][starts[0], envs[0]] = 1.0
        if n > 2:                                                  # ... and on the last frame only (valid = 1, dones = 1)
            host[3][starts[1]:starts[1] + n_frames, envs[1]] = 0.0
            host[3][starts[1] + n_frames - 1, envs[1]] = 1.0
        dev[3].copy_(torch.from_numpy(host[3]))
        want = SC.np_sample(*host, n_frames, starts, envs)
        if n > 2:
            assert want[5][1] == 1 and want[4][1] == 1 and (n_frames == 1 or want[5][0] == 0)
        for off in ((0, 4) if R == 36 else (0,)):
            six, index, _ = abi_sample(torch, *dev, n_frames, starts, envs, offset_states=off)
            SC.assert_six(six, want, f"R={R} n_frames={n_frames} E={E} n={n} offset={off}")
            assert np.array_equal(index, np.stack([starts, envs], axis=1))


# ------------------------------------------------------------------------------------------------------------- TurnBuffer layouts
@pytest.mark.parametrize("agent", [1, None])
@pytest.mark.parametrize("obs_dtype", ["uint8", "float32"])
def test_turnbuffer_layouts(torch_cuda, obs_dtype, agent):
    torch = torch_cuda
    from sorrel_amd.buffers import ReplaySampler

    ring, host = SC.turn_ring(torch, DEV, getattr(torch, obs_dtype))
    cap, E, A = host[1].shape
    R = 18
    cols = E * A if agent is None else E
    assert len(np.unique(host[0])) == 256                          # every byte value widens
    for n_frames in (1, 3):
        starts, envs = SC.turn_indices(cap, cols, n_frames)
        want = SC.turn_expected(host, agent, n_frames, starts, envs)
        ctx = f"{obs_dtype} agent={agent} n_frames={n_frames}"
        # the ring where it lies, through the ABI
        if agent is None:
            layout = dict(strides=((E * A * R, R), (E * A, 1)), offsets=(0, 0))
        else:
            layout = dict(strides=((E * A * R, A * R), (E * A, A)), offsets=(agent * R, agent))
        six, _, _ = abi_sample(torch, ring.obs, ring.actions, ring.rewards, ring.dones, n_frames, starts, envs, cols=cols, R=R, **layout)
        SC.assert_six(six, want, "sgw_sample " + ctx)
        assert six[1].dtype == np.int64
        # ... through TurnBuffer.sample and through a ReplaySampler
        got = ring.sample(len(starts), agent=agent, n_frames=n_frames, starts=starts, envs=envs)
        SC.assert_six(got, want, "TurnBuffer.sample " + ctx)
        assert got[1].dtype == torch.int64 and got[0].dtype == torch.float32
        sampler = ReplaySampler(ring, len(starts), n_frames=n_frames, agent=agent)
        SC.assert_six(sampler.sample(starts, envs), want, "ReplaySampler " + ctx)
        assert np.array_equal(sampler.last_index.cpu().numpy(), np.stack([starts, envs], axis=1))


@pytest.mark.parametrize("R", [36, 300, 75])
def test_uint8_rows(torch_cuda, R):
    """A uint8 ring whose rows are a multiple of four bytes takes the variant that loads a dword and stores 16 bytes (300: more
    than one pass of a wave's lanes is not needed, but lanes past the row's end are); 75 and a misplaced ``out_states`` take bytes."""
    torch = torch_cuda
    cap, E, n_frames, n = 24, 5, 2, 41
    rng = np.random.default_rng(R)
    states = rng.integers(0, 256, size=(cap, E, R)).astype(np.uint8)
    actions = rng.integers(0, 256, size=(cap, E)).astype(np.uint8)
    rewards = rng.integers(-9, 10, size=(cap, E)).astype(np.float32)
    dones = (rng.random((cap, E)) < 0.15).astype(np.float32)
    host = (states, actions, rewards, dones)
    starts, envs = indices(rng, n, cap - n_frames - 1, E)
    want = SC.np_sample(*host, n_frames, starts, envs)
    for off in (0, 4):
        six, _, _ = abi_sample(torch, *up(torch, host), n_frames, starts, envs, offset_states=off)
        SC.assert_six(six, want, f"uint8 R={R} offset={off}")


# ------------------------------------------------------------------------------------------------------------- grid-stride
def test_more_rows_than_waves(torch_cuda):
    """n * (n_frames + 1) rows exceed the waves of the largest grid the call launches: every wave takes a second row, some a third."""
    torch = torch_cuda
    R, n_frames, E, cap = 5, 1, 3, 24
    waves = SC.max_waves()
    n = waves + waves // 4 + 3                                    # 2 n rows = 2.5 x the waves, + 6
    assert n * (n_frames + 1) > 2 * waves
    rng = np.random.default_rng(77)
    host = f32_ring(rng, cap, E, R)
    starts, envs = indices(rng, n, cap - n_frames - 1, E)
    six, index, _ = abi_sample(torch, *up(torch, host), n_frames, starts, envs)
    SC.assert_six(six, SC.np_sample(*host, n_frames, starts, envs), "grid-stride")
    assert np.array_equal(index, np.stack([starts, envs], axis=1))


# ------------------------------------------------------------------------------------------------------------- indices out of range
def test_out_of_range_indices_leave_their_rows_unwritten(torch_cuda):
    torch = torch_cuda
    R, n_frames, E, cap = 75, 2, 3, 24
    num_starts = cap - n_frames - 1
    rng = np.random.default_rng(5)
    host = f32_ring(rng, cap, E, R)
    starts, envs = indices(rng, 12, num_starts, E)
    bad = {2: (-1, 0), 5: (num_starts, 1), 7: (3, E), 10: (4, -1)}
    for k, (t, e) in bad.items():
        starts[k], envs[k] = t, e
    six, index, outs = abi_sample(torch, *up(torch, host), n_frames, starts, envs)
    good = np.array([k for k in range(12) if k not in bad])
    want = SC.np_sample(*host, n_frames, starts[good], envs[good])
    SC.assert_six(tuple(a[good] for a in six), want, "the rows of good indices")
    assert np.array_equal(index[good], np.stack([starts[good], envs[good]], axis=1))
    for name, g in outs.items():
        raw = g.buf[g.lo:g.lo + g.total].cpu().numpy().reshape(12, -1)
        assert (raw[sorted(bad)] == 0xA5).all(), f"out_{name}: a row of an out-of-range index was written"


# ------------------------------------------------------------------------------------------------------------- drawn indices
def expected_draws(seed, counter, n, num_starts, num_envs):
    k = np.arange(n, dtype=np.uint64)
    kw = dict(env=counter >> 32, epoch=0, turn=counter & 0xFFFFFFFF, stream=9)
    starts = O.categorical(O.rng_u32(seed, index=2 * k, **kw), num_starts)
    envs = O.categorical(O.rng_u32(seed, index=2 * k + 1, **kw), num_envs)
    return np.stack([starts, envs], axis=1).astype(np.int64)


def test_drawn_indices_eager_and_in_a_replayed_graph(torch_cuda):
    torch = torch_cuda
    from sorrel_amd.buffers import Buffer, ReplaySampler

    E, cap, size, n_frames, B, R, seed = 7, 20, 15, 2, 33, 12, 0x1234_5678_9ABC_DEF1
    rng = np.random.default_rng(21)
    host = f32_ring(rng, cap, E, R)
    buf = Buffer(cap, (3, 2, 2), n_frames=n_frames, num_envs=E, device=DEV)
    for dst, src in zip((buf.states, buf.actions, buf.rewards, buf.dones), host):
        dst.copy_(torch.from_numpy(src).reshape(dst.shape))
    buf.idx = buf.size = size
    num_starts = size - n_frames - 1
    sampler = ReplaySampler(buf, B, seed=seed)
    assert sampler.n_frames == n_frames

    def check(counter, ctx):
        torch.cuda.synchronize()
        want_index = expected_draws(seed, counter, B, num_starts, E)
        assert want_index[:, 0].max() < num_starts and want_index[:, 1].max() < E
        assert np.array_equal(sampler.last_index.cpu().numpy(), want_index), ctx + ": the drawn (start, env) pairs"
        SC.assert_six(tuple(t.clone() for t in sampler.batch()), SC.np_sample(*host, n_frames, want_index[:, 0], want_index[:, 1]), ctx)

    for counter in (0, 1):
        got = sampler.sample()
        assert got[0].data_ptr() == sampler.batch()[0].data_ptr()      # views of the sampler's own storage
        check(counter, f"call {counter}")
    assert not np.array_equal(expected_draws(seed, 0, B, num_starts, E), expected_draws(seed, 1, B, num_starts, E))
    # the same draws through the bare ABI, from a host-side `draw` (no device counter)
    six, index, _ = abi_sample(torch, buf.states.view(cap, E, R), buf.actions, buf.rewards, buf.dones, n_frames, num_starts=num_starts, seed=seed, draw=1, n=B)
    assert np.array_equal(index, expected_draws(seed, 1, B, num_starts, E))
    SC.assert_six(six, SC.np_sample(*host, n_frames, index[:, 0], index[:, 1]), "draw = 1 through the ABI")
    # a counter with a high word: the 'env' slot of the Philox counter
    big = (5 << 32) | 7
    six, index, _ = abi_sample(torch, buf.states.view(cap, E, R), buf.actions, buf.rewards, buf.dones, n_frames, num_starts=num_starts, seed=seed, draw=big, n=B)
    assert np.array_equal(index, expected_draws(seed, big, B, num_starts, E))
    # recorded: a sampler that allocated, copied or synchronised would fail the capture; every replay draws anew
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sampler.sample()
    torch.cuda.synchronize()
    assert int(sampler.draw_count.cpu()[0]) == 2, "recording runs nothing"
    for counter in (2, 3):
        graph.replay()
        check(counter, f"replay with counter {counter}")
    assert int(sampler.draw_count.cpu()[0]) == 4


def test_recorded_sample_is_one_chain(torch_cuda):
    """What a capture of one ``sample()`` holds: the gather kernel, then the counter kernel -- two nodes, one edge, one root: no
    parallel branches."""
    torch = torch_cuda
    from sorrel_amd.buffers import Buffer, ReplaySampler

    buf = Buffer(12, (5,), n_frames=2, num_envs=3, device=DEV)
    buf.idx = buf.size = 12
    sampler = ReplaySampler(buf, 9, seed=3)
    sampler.sample()                                              # (code objects loaded before the capture)
    torch.cuda.synchronize()
    hip = C.CDLL(N._hip_runtimes_mapped()[0])                      # the runtime torch and libsgw.so share
    stream = torch.cuda.Stream()
    handle, graph = C.c_void_p(stream.cuda_stream), C.c_void_p()
    with torch.cuda.stream(stream):
        assert hip.hipStreamBeginCapture(handle, C.c_int(2)) == 0          # hipStreamCaptureModeRelaxed
        try:
            sampler.sample()
        finally:
            rc = hip.hipStreamEndCapture(handle, C.byref(graph))
    assert rc == 0 and graph.value
    nodes, edges, roots = C.c_size_t(), C.c_size_t(), C.c_size_t()
    assert hip.hipGraphGetNodes(graph, None, C.byref(nodes)) == 0
    assert hip.hipGraphGetEdges(graph, None, None, C.byref(edges)) == 0
    assert hip.hipGraphGetRootNodes(graph, None, C.byref(roots)) == 0
    assert hip.hipGraphDestroy(graph) == 0
    assert (nodes.value, edges.value, roots.value) == (2, 1, 1)
    torch.cuda.synchronize()
    assert int(sampler.draw_count.cpu()[0]) == 1, "a capture runs nothing"


# ------------------------------------------------------------------------------------------------------------- Buffer.sample keeps its contract
def test_buffer_sample_returns_tensors_the_caller_keeps(torch_cuda):
    torch = torch_cuda
    from sorrel_amd.buffers import Buffer

    E, cap, n_frames = 5, 16, 2
    rng = np.random.default_rng(8)
    host = f32_ring(rng, cap, E, 6)
    buf = Buffer(cap, (6,), n_frames=n_frames, num_envs=E, device=DEV)
    for dst, src in zip((buf.states, buf.actions, buf.rewards, buf.dones), host):
        dst.copy_(torch.from_numpy(src).reshape(dst.shape))
    buf.idx, buf.size = 0, cap
    torch.manual_seed(11)
    first = buf.sample(5)
    kept = [t.clone() for t in first]
    second = buf.sample(5)
    torch.cuda.synchronize()
    assert all(a.data_ptr() != b.data_ptr() for a, b in zip(first, second))
    assert all(torch.equal(a, b) for a, b in zip(first, kept)), "the second call overwrote the first call's results"
    # the host's draws are what they were: starts, then envs, from torch's generator
    torch.manual_seed(11)
    hi = cap - n_frames - 1
    t0, e = torch.randint(0, hi, (5,)).numpy(), torch.randint(0, E, (5,)).numpy()
    SC.assert_six(first, SC.np_sample(*host, n_frames, t0, e), "Buffer.sample(5)")
    t1, e1 = torch.randint(0, hi, (5,)).numpy(), torch.randint(0, E, (5,)).numpy()
    SC.assert_six(second, SC.np_sample(*host, n_frames, t1, e1), "the second Buffer.sample(5)")
    with pytest.raises(IndexError):
        buf.sample(2, starts=[0, cap - n_frames + 1], envs=[0, 0])


# ------------------------------------------------------------------------------------------------------------- a ring on another device
def test_a_ring_on_a_device_that_is_not_the_current_one(torch_cuda):
    """``TurnBuffer.sample`` and ``returns()`` of a ring on ``cuda:1`` while ``cuda:0`` is current: the launch is made under the ring's
    device (its pointers and its stream belong there), the results are the host expectations, and the current device stays 0."""
    torch = torch_cuda
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two devices")
    from sorrel_amd.buffers import _returns_torch
    from tests import returns_common as RC

    torch.cuda.set_device(0)
    ring, host = SC.turn_ring(torch, "cuda:1", torch.float32)
    cap, E, A = host[1].shape
    starts, envs = SC.turn_indices(cap, E * A, 1)
    got = ring.sample(len(starts), starts=starts, envs=envs)
    assert all(t.device == ring.device for t in got)
    SC.assert_six(got, SC.turn_expected(host, None, 1, starts, envs), "TurnBuffer.sample on cuda:1 under cuda:0")
    res = ring.returns(0.9, normalize="column")
    raw = _returns_torch(torch.from_numpy(host[2]), torch.from_numpy(host[3]), 0.9, 0, cap).returns.numpy()
    assert np.array_equal(res.returns.cpu().numpy(), raw)
    flat = raw.reshape(cap, E * A)
    RC.assert_normalized(res.normalized.cpu().numpy().reshape(cap, E * A), RC.host_normalized(flat, "column")[0], RC.tolerance(flat, axis=0),
                         "returns() on cuda:1 under cuda:0")
    assert torch.cuda.current_device() == 0
