"""``sgw_returns`` on the device: the reference's trajectories (``tests/golden/returns``) laid into rings among random columns, through the
C ABI and through ``Buffer`` / ``RolloutBuffer`` / ``TurnBuffer.returns``; a grid of column counts, segment lengths around the pipeline's
chunk, wrapping segments and strides against ``_returns_torch`` on a CPU copy (itself pinned by the fixture in
``tests/test_returns_cpu.py``); the normalised outputs against host float64 statistics within the derived tolerance
(``tests/returns_common.py``); the bytes around every output; and a recorded call.  Raw returns are compared for equality; no expectation
comes from the kernel."""
import ctypes as C

import numpy as np
import pytest

from sorrel_amd import _native as N
from tests import returns_common as RC
from tests.gpu_common import torch_cuda  # noqa: F401
from tests.learner_common import DEV, Guarded

pytestmark = pytest.mark.gpu

K = RC.chunk()
FIX = RC.load_fixture()
MODES = {None: N.RETURNS_NORM_NONE, "column": N.RETURNS_NORM_COLUMN, "all": N.RETURNS_NORM_ALL}


def abi_returns(torch, rewards, dones, *, first, count, capacity, cols, strides, offset=0, gamma, mode=None, f32=False, stats=True):
    """One ``sgw_returns`` call over device tensors ``rewards`` / ``dones``, read as the caller describes; every output and the workspace
    sit inside guards, which must come back untouched.  Returns (returns, normalized or None, stats or None)."""
    lib = N.load()
    out = Guarded(torch, (count, cols), np.float32)
    norm = Guarded(torch, (count, cols), np.float32 if f32 else np.float64) if mode else None
    st = Guarded(torch, (cols, 2) if mode == "column" else (2,), np.float64) if mode and stats else None
    need = int(lib.sgw_returns_workspace_bytes(count, cols)) if mode == "all" else 0
    assert need >= 0
    work = Guarded(torch, (max(need, 8) // 8,), np.float64) if mode == "all" else None
    d = N.SgwReturnsDesc()
    d.rewards, d.dones = rewards.data_ptr() + 4 * offset, dones.data_ptr() + 4 * offset
    d.out_returns = out.ptr
    if norm is not None:
        d.out_normalized = norm.ptr
    if st is not None:
        d.out_stats = st.ptr
    if work is not None:
        d.workspace, d.workspace_bytes = work.ptr, need
    d.first, d.count, d.capacity, d.cols = first, count, capacity, cols
    d.turn_stride, d.col_stride = strides
    d.gamma, d.normalize, d.out_type = gamma, MODES[mode], N.RETURNS_OUT_F32 if f32 else N.RETURNS_OUT_F64
    N.check(lib.sgw_returns(C.byref(d), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    for name, g in (("out_returns", out), ("out_normalized", norm), ("out_stats", st), ("workspace", work)):
        assert g is None or g.intact(), f"bytes around {name} were written"
    return out.numpy(), None if norm is None else norm.numpy(), None if st is None else st.numpy()


def cpu_returns(torch, rewards, dones, gamma, first, count):
    """``_returns_torch`` on host arrays ``[capacity, cols]``: what every raw result is compared with."""
    from sorrel_amd.buffers import _returns_torch

    return _returns_torch(torch.from_numpy(rewards), torch.from_numpy(dones), gamma, first, count).returns.numpy()


def check_normalized(raw, norm, stats, mode, ctx):
    """``norm`` / ``stats`` of the kernel against host float64 statistics (``math.fsum``) of the raw returns, within the derived tolerance;
    the mean and the std themselves within the same bound before its division by the std: ``8 n 2^-53 max|x|`` and ``8 n 2^-53 (std + max|x|)``."""
    want, mean, std = RC.host_normalized(raw, mode)
    tol = RC.tolerance(raw, axis=0 if mode == "column" else None)
    RC.assert_normalized(norm, want, tol, ctx)
    if stats is not None:
        x = np.abs(np.asarray(raw, np.float64))
        scale = x.max(axis=0) if mode == "column" else x.max()
        n = raw.shape[0] if mode == "column" else raw.size
        got_mean, got_std = (stats[:, 0], stats[:, 1]) if mode == "column" else (stats[0], stats[1])
        assert (np.abs(got_mean - mean) <= 8 * n * 2.0 ** -53 * scale).all(), f"{ctx}: out_stats mean"
        if n == 1:
            assert np.isnan(got_std).all(), f"{ctx}: the std of one value is NaN"
        else:
            assert (np.abs(got_std - std) <= 8 * n * 2.0 ** -53 * (std + scale)).all(), f"{ctx}: out_stats std"


# ------------------------------------------------------------------------------------------------------------- the reference's columns
@pytest.mark.parametrize("f", FIX, ids=[f"T{f['T']}-gamma{f['gamma']}" for f in FIX])
def test_fixture_columns_through_the_abi_and_the_rings(torch_cuda, f):
    torch = torch_cuda
    from sorrel_amd.buffers import Buffer, RolloutBuffer, TurnBuffer

    T, E, A = f["T"], 23, 3
    rng = np.random.default_rng(100 + T)
    cap = T + 2
    first = cap - max(1, T // 3)                                  # the segment wraps (T >= 2)
    planted = [(0, f["rewards"], f["dones"]), (E * A - 1, f["rewards"], 3.0 * f["dones"]), (31, f["rewards"], f["dones"])]
    rewards, dones = RC.ring_arrays(rng, cap, E * A, first, T, planted)
    want = cpu_returns(torch, rewards, dones, f["gamma"], first, T)
    dr, dd = torch.from_numpy(rewards).to(DEV), torch.from_numpy(dones).to(DEV)

    def check(raw, norm, ctx, cols):
        assert np.array_equal(raw, want[:, cols]), f"{ctx}: raw returns differ from the CPU path"
        for j, c in enumerate(cols):
            if c not in (0, E * A - 1, 31):
                continue
            assert np.array_equal(raw[:, j], f["returns"]), f"{ctx}: column {c} differs from the reference's returns"
            if T == 1:
                assert np.isnan(norm[:, j]).all(), f"{ctx}: one stored element normalises to NaN"
            else:
                RC.assert_normalized(norm[:, j], f["normalized"], RC.tolerance(f["returns"]), f"{ctx}: column {c} against the reference")

    every = list(range(E * A))
    raw, norm, _ = abi_returns(torch, dr, dd, first=first, count=T, capacity=cap, cols=E * A, strides=(E * A, 1), gamma=f["gamma"], mode="column")
    check(raw, norm, "sgw_returns", every)
    # a Buffer-shaped ring of E * A envs, a RolloutBuffer, and the TurnBuffer layouts
    for cls in (Buffer, RolloutBuffer):
        buf = cls(cap, (2,), num_envs=E * A, device=DEV)
        buf.rewards.copy_(dr)
        buf.dones.copy_(dd)
        buf.idx, buf.size = first, cap
        res = buf.returns(f["gamma"], normalize="column", first=first, count=T)
        check(res.returns.cpu().numpy(), res.normalized.cpu().numpy(), cls.__name__, every)
    ring = TurnBuffer(cap, E, (A, 1, 1, 1), device=DEV)
    ring.rewards.copy_(dr.view(cap, E, A))
    ring.dones.copy_(dd.view(cap, E, A))
    ring.idx, ring.size = first, cap
    res = ring.returns(f["gamma"], normalize="column", first=first, count=T)
    assert tuple(res.returns.shape) == (T, E, A) and tuple(res.mean.shape) == (E, A)
    check(res.returns.cpu().numpy().reshape(T, -1), res.normalized.cpu().numpy().reshape(T, -1), "TurnBuffer agent=None", every)
    for a in range(A):
        one = ring.returns(f["gamma"], agent=a, normalize="column", first=first, count=T)
        check(one.returns.cpu().numpy(), one.normalized.cpu().numpy(), f"TurnBuffer agent={a}", [e * A + a for e in range(E)])


# ------------------------------------------------------------------------------------------------------------- sizes
@pytest.mark.parametrize("col_stride", [1, 3])
@pytest.mark.parametrize("cols", [1, 63, 64, 65, 67, 600])
def test_sizes_against_the_cpu_path(torch_cuda, cols, col_stride):
    """Every segment length around the chunk, wrapping segments, a turn stride larger than the columns need; every mode and output type."""
    torch = torch_cuda
    gamma = 0.97
    rng = np.random.default_rng(1000 * cols + col_stride)
    for count in (1, 2, K - 1, K, K + 1, 2 * K + 3):
        cap = 2 * K + 5
        first = cap - 2 if count > 2 else cap - 1                    # near the end of the ring: every segment of two or more turns wraps
        width = cols * col_stride + 5                                  # a turn stride larger than the columns need
        offset = 2 if col_stride > 1 else 0
        rewards, dones = RC.random_columns(rng, cap, width)
        lanes = offset + col_stride * np.arange(cols)
        want = cpu_returns(torch, np.ascontiguousarray(rewards[:, lanes]), np.ascontiguousarray(dones[:, lanes]), gamma, first, count)
        dr, dd = torch.from_numpy(rewards).to(DEV), torch.from_numpy(dones).to(DEV)
        kw = dict(first=first, count=count, capacity=cap, cols=cols, strides=(width, col_stride), offset=offset, gamma=gamma)
        ctx = f"cols={cols} count={count} col_stride={col_stride}"
        raw, norm, stats = abi_returns(torch, dr, dd, **kw)
        assert np.array_equal(raw, want) and norm is None, f"{ctx}: raw returns"
        results = {}
        for mode in ("column", "all"):
            for f32 in (False, True):
                raw, norm, stats = abi_returns(torch, dr, dd, mode=mode, f32=f32, **kw)
                assert np.array_equal(raw, want), f"{ctx} {mode}: raw returns"
                results[mode, f32] = norm
                if mode == "all" or not f32:
                    check_normalized(want, norm, stats, mode, f"{ctx} {mode} f32={f32}")
        # float32 NORM_COLUMN: the float64 result rounded once
        assert np.array_equal(results["column", True], results["column", False].astype(np.float32), equal_nan=True), f"{ctx}: float32 column output"
        # without out_stats; and NORM_ALL twice: identical bits
        again = abi_returns(torch, dr, dd, mode="all", stats=False, **kw)[1]
        assert np.array_equal(again, results["all", False], equal_nan=True), f"{ctx}: two NORM_ALL runs differ"
        assert np.array_equal(abi_returns(torch, dr, dd, mode="column", stats=False, **kw)[1], results["column", False], equal_nan=True)


def test_more_column_tiles_than_workgroups(torch_cuda):
    """More tiles of 256 columns than the grid's cap: the workgroups stride, and NORM_ALL merges moments a lane carried across tiles."""
    torch = torch_cuda
    cols, count, cap, gamma = 256 * RC.max_blocks() + 300, 3, 4, 0.9
    rng = np.random.default_rng(9)
    rewards, dones = RC.random_columns(rng, cap, cols)
    want = cpu_returns(torch, rewards, dones, gamma, 2, count)
    dr, dd = torch.from_numpy(rewards).to(DEV), torch.from_numpy(dones).to(DEV)
    kw = dict(first=2, count=count, capacity=cap, cols=cols, strides=(cols, 1), gamma=gamma)
    raw, norm, stats = abi_returns(torch, dr, dd, mode="all", **kw)
    assert np.array_equal(raw, want)
    check_normalized(want, norm, stats, "all", "strided tiles, all")
    raw, norm, stats = abi_returns(torch, dr, dd, mode="column", **kw)
    assert np.array_equal(raw, want)
    edge = 256 * RC.max_blocks()                                       # (the statistics of the first tile, of the columns around the first
    sel = np.r_[0:256, edge - 64:cols]                                 #  tile a workgroup takes second, and of the last, partial tile)
    check_normalized(want[:, sel], norm[:, sel], stats[sel], "column", "strided tiles, column")


def test_done_is_tested_by_truthiness_and_no_turns_launch_nothing(torch_cuda):
    torch = torch_cuda
    rewards = np.float32([[1.0, 1.0, 1.0, 1.0]] * 3)
    dones = np.zeros((3, 4), np.float32)
    dones[1] = (0.0, -2.5, np.nan, 1e-30)                             # any non-zero value ends the episode, as `if done:` does
    dr, dd = torch.from_numpy(rewards).to(DEV), torch.from_numpy(dones).to(DEV)
    raw, _, _ = abi_returns(torch, dr, dd, first=0, count=3, capacity=3, cols=4, strides=(4, 1), gamma=0.5)
    assert raw[:, 0].tolist() == [1.75, 1.5, 1.0] and all(raw[:, c].tolist() == [1.5, 1.0, 1.0] for c in (1, 2, 3))
    assert np.array_equal(raw, cpu_returns(torch, rewards, dones, 0.5, 0, 3))
    out = torch.full((8,), 7.0, device=DEV)
    d = N.SgwReturnsDesc()
    d.rewards, d.dones, d.out_returns = dr.data_ptr(), dd.data_ptr(), out.data_ptr()
    d.first, d.count, d.capacity, d.cols, d.turn_stride, d.col_stride, d.gamma = 0, 0, 3, 4, 4, 1, 0.5
    N.check(N.load().sgw_returns(C.byref(d), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# ------------------------------------------------------------------------------------------------------------- recorded
@pytest.mark.parametrize("mode", [None, "column", "all"])
def test_recorded_returns_replay_on_new_rewards(torch_cuda, mode):
    """A captured ``returns(out=res)`` allocates nothing and does not synchronise (either would fail the capture); replayed after
    the rewards changed it equals an eager call."""
    torch = torch_cuda
    from sorrel_amd.buffers import TurnBuffer

    E, A, cap, gamma = 67, 3, 2 * K + 3, 0.97
    rng = np.random.default_rng(31)
    ring = TurnBuffer(cap, E, (A, 1, 1, 1), device=DEV)
    rewards, dones = RC.random_columns(rng, cap, E * A)
    ring.rewards.copy_(torch.from_numpy(rewards).view(cap, E, A))
    ring.dones.copy_(torch.from_numpy(dones).view(cap, E, A))
    ring.idx, ring.size = 5, cap
    res = ring.returns(gamma, normalize=mode, dtype=torch.float32)     # (code objects loaded before the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        assert ring.returns(gamma, normalize=mode, dtype=torch.float32, out=res) is res
    torch.cuda.synchronize()
    rewards2, _ = RC.random_columns(rng, cap, E * A)
    assert not np.array_equal(rewards, rewards2)
    ring.rewards.copy_(torch.from_numpy(rewards2).view(cap, E, A))
    res.returns.fill_(-1.0)
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(res.returns.cpu().numpy().reshape(cap, -1), cpu_returns(torch, rewards2, dones, gamma, 5, cap))
    eager = ring.returns(gamma, normalize=mode, dtype=torch.float32)
    torch.cuda.synchronize()
    assert eager.returns.data_ptr() != res.returns.data_ptr() and torch.equal(eager.returns, res.returns)
    if mode:
        assert torch.equal(eager.normalized, res.normalized) and torch.equal(eager.mean, res.mean) and torch.equal(eager.std, res.std)


def test_recorded_norm_all_is_one_chain(torch_cuda):
    """What a capture of one ``normalize="all"`` call holds: the returns kernel, then the kernel that merges the partials and
    normalises -- two nodes, one edge, one root: no parallel branches."""
    torch = torch_cuda
    from sorrel_amd.buffers import Buffer

    buf = Buffer(12, (2,), num_envs=600, device=DEV)
    buf.rewards.copy_(torch.arange(12 * 600, device=DEV).view(12, 600) % 7)
    buf.idx, buf.size = 0, 12
    res = buf.returns(0.9, normalize="all")
    torch.cuda.synchronize()
    hip = C.CDLL(N._hip_runtimes_mapped()[0])                      # the runtime torch and libsgw.so share
    stream = torch.cuda.Stream()
    handle, graph = C.c_void_p(stream.cuda_stream), C.c_void_p()
    with torch.cuda.stream(stream):
        assert hip.hipStreamBeginCapture(handle, C.c_int(2)) == 0          # hipStreamCaptureModeRelaxed
        try:
            buf.returns(0.9, normalize="all", out=res)
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
