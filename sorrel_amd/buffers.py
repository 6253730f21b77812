"""Batched replay ring on the device: the consumer of the step's outputs
(``sorrel/buffers.py:11-154``).

One ring slot holds one turn of one agent for ALL ``num_envs`` envs, so ``add`` is a
single device-to-device copy of the kernel's output tensors (no 617 MB/step PCIe
round trip).  dtypes follow the reference: states float32, actions int64, rewards
float32, dones float32 (``sorrel/buffers.py:31-34``)."""
from __future__ import annotations

from pathlib import Path
from typing import Sequence

import numpy as np
import torch

from sorrel_amd.spec import resolve_device


def _stack_torch(states, actions, rewards, dones, n_frames: int, batch_size: int, t0, e):
    """The reference's stacking (``sorrel/buffers.py:109-122``) over a ring ``[capacity, N, ...]`` by torch indexing."""
    device = states.device
    t0 = torch.as_tensor(t0, dtype=torch.long)
    e = torch.as_tensor(e, dtype=torch.long).to(device)
    idx = (t0.cpu()[:, None] + torch.arange(n_frames)[None, :]).to(device)        # [B, n_frames]
    ee = e[:, None].expand_as(idx)
    src = states[idx, ee].reshape(batch_size, -1)
    nxt = states[idx + 1, ee].reshape(batch_size, -1)
    last = idx[:, -1]
    acts = actions[last, e].reshape(batch_size, -1)
    rews = rewards[last, e].reshape(batch_size, -1)
    dns = dones[last, e].reshape(batch_size, -1)
    valid = (1.0 - (dones[idx[:, :-1], ee[:, :-1]] != 0).any(dim=-1).float()).reshape(batch_size, -1)
    return src, acts, rews, nxt, dns, valid


def _ring_layout(ring, agent):
    """What ``sgw_sample`` needs to read a ring where it lies: base pointers, the number of (env) columns, the row length, the
    (turn, env) strides of the rows and of the scalars, and the element types (include/sgw.h)."""
    from sorrel_amd import _native as N

    if isinstance(ring, TurnBuffer):
        E, A = ring.num_envs, ring.obs_shape[0]
        R = int(np.prod(ring.obs_shape[1:]))
        if ring.obs.dtype not in (torch.float32, torch.uint8):
            raise TypeError(f"sgw_sample reads float32 or uint8 observations, not {ring.obs.dtype}")
        src = N.SAMPLE_U8 if ring.obs.dtype == torch.uint8 else N.SAMPLE_F32
        tensors = (ring.obs, ring.actions, ring.rewards, ring.dones)
        if agent is None:
            cols, offs, sstr, cstr = E * A, (0, 0), (E * A * R, R), (E * A, 1)
        else:
            if not 0 <= int(agent) < A:
                raise IndexError(f"agent {agent} outside [0, {A})")
            cols, offs, sstr, cstr = E, (int(agent) * R, int(agent)), (E * A * R, A * R), (E * A, A)
        act = N.SAMPLE_ACT_U8
    else:
        if agent is not None:
            raise ValueError("a Buffer holds one agent: agent must be None")
        E, R = ring.num_envs, int(np.prod(ring.obs_shape))
        tensors = (ring.states, ring.actions, ring.rewards, ring.dones)
        cols, offs, sstr, cstr = E, (0, 0), (E * R, R), (E, 1)
        src, act = N.SAMPLE_F32, N.SAMPLE_ACT_I64
    for t in tensors:
        if not t.is_contiguous():
            raise ValueError("sgw_sample reads contiguous rings")
    st, ac, rw, dn = tensors
    ptrs = (st.data_ptr() + offs[0] * st.element_size(), ac.data_ptr() + offs[1] * ac.element_size(),
            rw.data_ptr() + offs[1] * 4, dn.data_ptr() + offs[1] * 4)
    return dict(ptrs=ptrs, cols=cols, R=R, sstr=sstr, cstr=cstr, src=src, act=act, capacity=ring.capacity, device=ring.device)


def _check_index_list(name, values, batch_size, bound, device):
    """A caller's index list: host values are range-checked (``IndexError``), device tensors passed through as they are."""
    if torch.is_tensor(values) and values.device.type == "cuda":
        out = values.to(device=device, dtype=torch.long).contiguous()
        if out.numel() != batch_size:
            raise ValueError(f"{name}: {out.numel()} indices for a batch of {batch_size}")
        return out
    host = np.asarray(values.cpu() if torch.is_tensor(values) else values).astype(np.int64).reshape(-1)
    if host.size != batch_size:
        raise ValueError(f"{name}: {host.size} indices for a batch of {batch_size}")
    if host.size and (host.min() < 0 or host.max() >= bound):
        raise IndexError(f"{name}: index outside [0, {bound})")
    return host


def _launch_sample(layout, n_frames, batch_size, outs, index, starts, envs, num_starts, count=None, seed=0, clock=None):
    """One ``sgw_sample`` call on the current stream.  ``outs`` = (states, next_states, actions, rewards, dones, valid) tensors.
    ``clock`` (the device address of an ``sgw_learn_clock``): ``sgw_sample_clocked``, with ``num_starts`` the upper bound of the clock's."""
    from sorrel_amd import _native as N

    d = N.SgwSampleDesc()
    d.states, d.actions, d.rewards, d.dones = layout["ptrs"]
    if starts is not None:
        d.starts, d.envs = starts.data_ptr(), envs.data_ptr()
    if count is not None:
        d.draw_count = count.data_ptr()
    d.out_states, d.out_next_states, d.out_actions, d.out_rewards, d.out_dones, d.out_valid = (t.data_ptr() for t in outs)
    if index is not None:
        d.out_index = index.data_ptr()
    d.n, d.capacity, d.num_envs, d.num_starts, d.row_elems = batch_size, layout["capacity"], layout["cols"], num_starts, layout["R"]
    d.state_turn_stride, d.state_env_stride = layout["sstr"]
    d.scalar_turn_stride, d.scalar_env_stride = layout["cstr"]
    d.seed, d.draw = seed & 0xFFFFFFFFFFFFFFFF, 0
    d.n_frames, d.src_type, d.act_type = n_frames, layout["src"], layout["act"]
    N.launch("sgw_sample", d, layout["device"], clock=clock)


def _sample_outputs(batch_size, n_frames, R, device):
    f32 = dict(dtype=torch.float32, device=device)
    return (torch.empty((batch_size, n_frames * R), **f32), torch.empty((batch_size, n_frames * R), **f32),
            torch.empty((batch_size, 1), dtype=torch.int64, device=device), torch.empty((batch_size, 1), **f32),
            torch.empty((batch_size, 1), **f32), torch.empty((batch_size, 1), **f32))


def _sample_fresh(layout, n_frames, batch_size, t0, e, num_starts):
    """Host-side indices -> one upload -> ``sgw_sample`` into freshly allocated tensors (``Buffer.sample`` / ``TurnBuffer.sample``
    on a device ring): the caller keeps the results."""
    device = layout["device"]
    t0 = _check_index_list("starts", t0, batch_size, num_starts, device)
    e = _check_index_list("envs", e, batch_size, layout["cols"], device)
    if isinstance(t0, np.ndarray) and isinstance(e, np.ndarray):
        both = torch.from_numpy(np.stack([t0, e])).to(device)
        t0, e = both[0], both[1]
    else:
        t0 = torch.from_numpy(t0).to(device) if isinstance(t0, np.ndarray) else t0
        e = torch.from_numpy(e).to(device) if isinstance(e, np.ndarray) else e
    outs = _sample_outputs(batch_size, n_frames, layout["R"], device)
    if batch_size:
        _launch_sample(layout, n_frames, batch_size, outs, None, t0, e, num_starts)
    s, ns, a, r, dn, v = outs
    return s, a, r, ns, dn, v


class Returns:
    """What ``Buffer.returns`` / ``TurnBuffer.returns`` give back: ``returns`` float32 ``[count, E]`` (``[count, E, A]`` over every agent
    of a ``TurnBuffer``), row 0 the oldest turn of the segment; ``normalized`` of the asked dtype and ``mean`` / ``std`` (float64: one
    value per column for ``normalize="column"``, 0-d tensors for ``"all"``) or None without normalisation.  Passed back as ``out=``
    its tensors are overwritten in place."""

    __slots__ = ("returns", "normalized", "mean", "std", "_stats", "_workspace", "_mode")

    def __init__(self, shape, normalize, dtype, device):
        from sorrel_amd import _native as N

        cols = int(np.prod(shape[1:]))
        self._mode = normalize
        self.returns = torch.empty(shape, dtype=torch.float32, device=device)
        self.normalized = self.mean = self.std = self._stats = self._workspace = None
        if normalize is not None:
            self.normalized = torch.empty(shape, dtype=dtype, device=device)
            self._stats = torch.empty((cols, 2) if normalize == "column" else (2,), dtype=torch.float64, device=device)
            self.mean = self._stats[..., 0].view(shape[1:] if normalize == "column" else ())
            self.std = self._stats[..., 1].view(shape[1:] if normalize == "column" else ())
        if normalize == "all" and torch.device(device).type == "cuda":
            self._workspace = N.workspace(N.load().sgw_returns_workspace_bytes(max(int(shape[0]), 1), cols), device)

    def __repr__(self):
        return f"Returns(shape={tuple(self.returns.shape)}, normalize={self._mode!r})"


def _returns_result(shape, normalize, dtype, device, out):
    """A fresh ``Returns``, or the caller's ``out`` after checking that it was made for this call's shape and mode."""
    if normalize not in (None, "column", "all"):
        raise ValueError(f"normalize must be None, 'column' or 'all', not {normalize!r}")
    if dtype not in (torch.float64, torch.float32):
        raise TypeError(f"normalised returns are float64 or float32, not {dtype}")
    if out is None:
        return Returns(shape, normalize, dtype, device)
    if not isinstance(out, Returns) or tuple(out.returns.shape) != tuple(shape) or out._mode != normalize or out.returns.device != torch.device(device) \
            or (normalize is not None and out.normalized.dtype != dtype):
        raise ValueError(f"out= was not made by a returns() call of shape {tuple(shape)}, normalize={normalize!r}, dtype={dtype} on {device}")
    return out


def _returns_torch(rewards, dones, gamma, first, count, normalize=None, dtype=torch.float64, out=None):
    """The reference's returns (``sorrel/models/pytorch/ppo.py:226-239``) by torch calls: the path of CPU rings, and what ``sgw_returns`` is
    compared with and timed against.  ``rewards`` / ``dones`` are ``[capacity, ...]`` views of a ring; the recurrence runs backwards over
    ``count`` rows from row ``first`` (wrapping), one turn of every column per round, in float32 with the product and the sum rounded
    separately -- a multiply, then an add -- which is the reference's arithmetic bit for bit."""
    import warnings

    capacity = int(rewards.shape[0])
    res = _returns_result((count,) + tuple(rewards.shape[1:]), normalize, dtype, rewards.device, out)
    g = torch.tensor(gamma, dtype=torch.float32, device=rewards.device)          # NumPy rounds the Python float to float32 as well
    d = torch.zeros(tuple(rewards.shape[1:]), dtype=torch.float32, device=rewards.device)
    for t in range(count - 1, -1, -1):
        row = (first + t) % capacity
        d = d.masked_fill(dones[row] != 0, 0.0)
        d = torch.add(rewards[row], torch.mul(d, g), out=res.returns[t])
    if normalize is not None:
        x = res.returns.to(torch.float64)
        dim = 0 if normalize == "column" else None
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")              # (one value: torch warns, and gives NaN as the reference does)
            mean, std = x.mean(dim=dim), x.std(dim=dim)
        res.mean.copy_(mean)
        res.std.copy_(std)
        res.normalized.copy_((x - mean) / (std + 1e-7))
    return res


def _returns_views(ring, agent):
    """``rewards`` / ``dones`` of a ring as ``[capacity, columns...]`` views, and how ``sgw_returns`` reads the same columns where they
    lie: the element offset of column 0 and the (turn, column) strides."""
    if isinstance(ring, TurnBuffer):
        E, A = ring.num_envs, ring.obs_shape[0]
        if agent is None:
            return ring.rewards, ring.dones, 0, (E * A, 1)
        if not 0 <= int(agent) < A:
            raise IndexError(f"agent {agent} outside [0, {A})")
        return ring.rewards[:, :, int(agent)], ring.dones[:, :, int(agent)], int(agent), (E * A, A)
    if agent is not None:
        raise ValueError("a Buffer holds one agent: agent must be None")
    return ring.rewards, ring.dones, 0, (ring.num_envs, 1)


def _ring_returns(ring, agent, gamma, normalize, first, count, dtype, out):
    """``returns()`` of both ring classes: the segment's defaults and bounds, then ``sgw_returns`` (device ring) or ``_returns_torch``."""
    cap = ring.capacity
    full = ring.size >= cap
    if first is None:
        first = ring.idx if full else 0
    if count is None:
        count = ((ring.idx - first) % cap or cap) if full else max(ring.size - first, 0)          # from `first` to the newest row
    first, count = int(first), int(count)
    if not 0 <= first < cap or not 0 <= count <= cap:
        raise ValueError(f"returns over rows first={first}, count={count} of a ring of {cap}")
    rewards, dones, offset, (ts, cs) = _returns_views(ring, agent)
    if ring.device.type != "cuda":
        return _returns_torch(rewards, dones, gamma, first, count, normalize, dtype, out)
    from sorrel_amd import _native as N

    for t in (ring.rewards, ring.dones):
        if not t.is_contiguous():
            raise ValueError("sgw_returns reads contiguous rings")
    res = _returns_result((count,) + tuple(rewards.shape[1:]), normalize, dtype, ring.device, out)
    d = N.SgwReturnsDesc()
    d.rewards, d.dones = ring.rewards.data_ptr() + 4 * offset, ring.dones.data_ptr() + 4 * offset
    d.out_returns = res.returns.data_ptr()
    if normalize is not None:
        d.out_normalized, d.out_stats = res.normalized.data_ptr(), res._stats.data_ptr()
    if res._workspace is not None:
        d.workspace, d.workspace_bytes = res._workspace.data_ptr(), res._workspace.numel() * 8
    d.first, d.count, d.capacity, d.cols = first, count, cap, int(np.prod(rewards.shape[1:]))
    d.turn_stride, d.col_stride = ts, cs
    d.gamma = float(gamma)
    d.normalize = {None: N.RETURNS_NORM_NONE, "column": N.RETURNS_NORM_COLUMN, "all": N.RETURNS_NORM_ALL}[normalize]
    d.out_type = N.RETURNS_OUT_F32 if dtype == torch.float32 else N.RETURNS_OUT_F64
    N.launch("sgw_returns", d, ring.device)
    return res


class Buffer:
    """``extra`` keyword arguments declare additional int64 columns exactly as in the reference
    (``Buffer(capacity, obs_shape, positions=(2,))``, ``sorrel/buffers.py:39-44``): a tuple gives the trailing
    shape, anything else a scalar column; ``add(..., positions=...)`` fills them."""

    def __init__(self, capacity: int, obs_shape: Sequence[int], n_frames: int = 1, num_envs: int = 1, device=None,
                 **extra):
        self.capacity, self.obs_shape, self.n_frames, self.num_envs = capacity, tuple(obs_shape), n_frames, num_envs
        self.device = resolve_device(device)
        E = num_envs
        self.states = torch.zeros((capacity, E, *self.obs_shape), dtype=torch.float32, device=self.device)
        self.actions = torch.zeros((capacity, E), dtype=torch.int64, device=self.device)
        self.rewards = torch.zeros((capacity, E), dtype=torch.float32, device=self.device)
        self.dones = torch.zeros((capacity, E), dtype=torch.float32, device=self.device)
        self.idx = 0
        self.size = 0
        self._prefilled = None        # (row, data_ptr of the action tensor): sgw_act already wrote that action into actions[row]
        self._dones_dirty = False     # some dones row may be non-zero (a done was stored, or rows were copied / loaded in): until then
                                      # the rows are all zero already and add(done=False) has nothing to write
        self._deferred = False        # a captured policy turn is being recorded / replayed: the engine's own kernels fill the row
        self._deferred_adds = 0       # (device-side row count, sgw_turn_end) -- add() only keeps the host's idx / size in step
        self._prev_rows = None        # ... and current_state() is gathered on the device by that same count (sgw_turn_prev_rows)
        self.extra_data = {}
        for key, value in extra.items():
            shape = (capacity, E, *value) if isinstance(value, tuple) else (capacity, E)
            self.extra_data[key] = torch.zeros(shape, dtype=torch.int64, device=self.device)

    def add(self, obs, action, reward, done, **extra):
        """Append one turn: ``obs [E, *obs_shape]``, ``action [E]``, ``reward [E]``, ``done`` scalar or ``[E]``.
        Whatever the kernels have already written where it belongs is not copied again: the state (a window rendered
        straight into this row), the reward (``sgw_act``'s ``reward_row``) and the action (``sgw_act``'s ``action_row``,
        announced through ``_prefilled``)."""
        if self._deferred:
            self._deferred_adds += 1
            self.idx = (self.idx + 1) % self.capacity
            self.size = min(self.size + 1, self.capacity)
            return
        i = self.idx
        row = self.states[i]
        src = obs.reshape(row.shape)
        if src.data_ptr() != row.data_ptr():       # (the step kernel may have written the state straight into this row)
            row.copy_(src)
        pre, self._prefilled = self._prefilled, None
        if not (pre is not None and pre[0] == i and torch.is_tensor(action) and action.data_ptr() == pre[1]):
            self.actions[i].copy_(action)
        if not (torch.is_tensor(reward) and reward.data_ptr() == self.rewards[i].data_ptr() and reward.dtype == torch.float32):
            self.rewards[i].copy_(reward)
        if torch.is_tensor(done) or done:
            self.dones[i] = done
            self._dones_dirty = True
        elif self._dones_dirty:
            self.dones[i] = 0
        for key, value in extra.items():
            self.extra_data[key][i] = torch.as_tensor(value, device=self.device)
        self.idx = (self.idx + 1) % self.capacity
        self.size = min(self.size + 1, self.capacity)

    def add_batch(self, obs, actions, rewards, done=False) -> None:
        """``k`` consecutive ``add`` calls at once -- ``obs [k, E, *obs_shape]``, ``actions`` / ``rewards`` ``[k, E]`` -- as the agents
        that share this buffer would have made them in list order (``sorrel/buffers.py:46-63``: row ``idx``, ``idx + 1``, ...,
        wrapping around): three copies instead of ``3 k``."""
        k = int(obs.shape[0])
        if k > self.capacity:
            raise ValueError(f"add_batch of {k} rows into a ring of {self.capacity}")
        if self._deferred:
            raise RuntimeError("add_batch inside a recorded turn")
        per_row = torch.is_tensor(done) and done.dim() == 2          # [k, E]: a flag per row; a scalar or [E] broadcasts over the rows
        if per_row and tuple(done.shape) != (k, self.num_envs):        # (checked before anything is written: the ring stays consistent)
            raise ValueError(f"done must be a scalar, [{self.num_envs}] or [{k}, {self.num_envs}]; got {tuple(done.shape)}")
        first = min(k, self.capacity - self.idx)
        for lo, hi, at in ((0, first, self.idx), (first, k, 0)):
            if hi <= lo:
                continue
            n = hi - lo
            if obs[lo].data_ptr() != self.states[at].data_ptr():          # (the windows may have been rendered straight into these rows)
                self.states[at:at + n].copy_(obs[lo:hi].reshape((n,) + tuple(self.states.shape[1:])))
            self.actions[at:at + n].copy_(actions[lo:hi])
            self.rewards[at:at + n].copy_(rewards[lo:hi])
            if torch.is_tensor(done) or done:
                self.dones[at:at + n] = done[lo:hi] if per_row else done     # (a wrap-around splits the rows: each segment takes ITS flags)
                self._dones_dirty = True
            elif self._dones_dirty:
                self.dones[at:at + n] = 0
        self.idx = (self.idx + k) % self.capacity
        self.size = min(self.size + k, self.capacity)

    def add_from_buffer(self, buffer: "Buffer") -> None:
        """Append the first ``min(capacity - idx, buffer.size)`` rows of another buffer, the reference's
        ``add_from_buffer`` exactly (``sorrel/buffers.py:71-99``): no wrap-around, ``idx`` only advances, ``size``
        is left alone; extra columns the source carries are created on demand."""
        if tuple(self.obs_shape) != tuple(buffer.obs_shape):
            raise AssertionError("Cannot add from a buffer with different state shapes.")
        n = min(self.capacity - self.idx, buffer.size)
        lo, hi = self.idx, self.idx + n
        self.states[lo:hi].copy_(buffer.states[:n])
        self.actions[lo:hi].copy_(buffer.actions[:n])
        self.rewards[lo:hi].copy_(buffer.rewards[:n])
        self.dones[lo:hi].copy_(buffer.dones[:n])
        for key, value in buffer.extra_data.items():
            if key not in self.extra_data:
                self.extra_data[key] = torch.zeros((self.capacity, *value.shape[1:]), dtype=value.dtype, device=self.device)
            self.extra_data[key][lo:hi].copy_(value[:n])
        self.idx = hi
        self._dones_dirty = True      # (the copied rows may hold terminal flags: later add(done=False) must clear them)

    # -- files: the reference's ``Buffer.save`` / ``Buffer.load`` format (``sorrel/buffers.py:168-201``)
    def _file_arrays(self) -> dict:
        """One env: exactly the reference's arrays (all ``capacity`` rows, scalar ``idx``).  Several envs: the rows
        of env ``e`` follow those of env ``e - 1`` (each block = that env's ring in storage order, what the reference
        would have saved for that one world), plus ``num_envs`` so that ``load`` can fold them back; a reader that
        does not know about batches (the reference's ``Buffer.load``) sees one long valid buffer."""
        E = self.num_envs

        def flat(t):
            t = t.detach().cpu()
            return t.transpose(0, 1).reshape((E * self.capacity,) + tuple(t.shape[2:])).contiguous().numpy()

        out = dict(states=flat(self.states), actions=flat(self.actions), rewards=flat(self.rewards), dones=flat(self.dones),
                   n_frames=self.n_frames, idx=self.idx if E == 1 else E * self.idx)
        for key, value in self.extra_data.items():
            out[key] = flat(value)
        if E > 1:
            out["num_envs"] = E
        return out

    def save(self, output_file) -> None:
        arrays = self._file_arrays()
        arrays = {k: v for k, v in arrays.items() if k in ("states", "actions", "rewards", "dones", "n_frames", "idx", "num_envs")}
        np.savez_compressed(Path(output_file), **arrays)

    @classmethod
    def load(cls, input_file, device="cpu") -> "Buffer":
        """Reads files written by this class or by the reference's ``Buffer.save`` / ``SavedGames.save``; like the
        reference, the loaded buffer counts as full (``size = len(states)`` per env)."""
        with np.load(Path(input_file)) as data:
            arrays = {k: data[k] for k in data.files}
        E = int(arrays.pop("num_envs", 1))
        n_frames, idx = int(arrays.pop("n_frames")), int(arrays.pop("idx"))
        rows = len(arrays["actions"]) // E
        extra = {k: tuple(v.shape[1:]) or None for k, v in arrays.items() if k not in ("states", "actions", "rewards", "dones")}
        out = cls(capacity=rows, obs_shape=arrays["states"].shape[1:], n_frames=n_frames, num_envs=E, device=device,
                  **{k: (v if v is not None else 0) for k, v in extra.items()})

        def fold(a, like):
            t = torch.from_numpy(np.ascontiguousarray(a)).reshape((E, rows) + tuple(a.shape[1:])).transpose(0, 1)
            return t.to(device=like.device, dtype=like.dtype).contiguous()

        out.states, out.actions = fold(arrays["states"], out.states), fold(arrays["actions"], out.actions)
        out.rewards, out.dones = fold(arrays["rewards"], out.rewards), fold(arrays["dones"], out.dones)
        for k in extra:
            out.extra_data[k] = fold(arrays[k], out.extra_data[k])
        out.idx = idx if E == 1 else idx // E
        out.size = rows
        out._dones_dirty = True       # loaded rows may hold terminal flags
        return out

    def __len__(self):
        return self.size

    def __getitem__(self, i):
        return self.states[i], self.actions[i], self.rewards[i], self.dones[i]

    def add_empty(self):
        self.idx = (self.idx + self.n_frames - 1) % self.capacity
        self.size = min(self.size + 1, self.capacity)

    def clear(self):
        for t in (self.states, self.actions, self.rewards, self.dones, *self.extra_data.values()):
            t.zero_()
        self.idx = self.size = 0
        self._dones_dirty = False

    def getidx(self):
        return self.idx

    def current_state(self) -> torch.Tensor:
        """The last ``n_frames - 1`` stored observations ``[n_frames-1, E, *obs_shape]``
        (``sorrel/buffers.py:143-154``), wrapping around the ring."""
        k = self.n_frames - 1
        if k == 0:
            return self.states[0:0]
        if self._deferred and self._prev_rows is not None:       # a recorded turn: the engine gathers by its own row count
            return self._prev_rows()
        sel = [(self.idx - k + j) % self.capacity for j in range(k)]
        return self.states[sel]

    def _draw(self, batch_size: int, starts, envs):
        """The host's draws (or the caller's indices): ``starts`` before ``envs``, from torch's global generator."""
        hi = max(1, self.size - self.n_frames - 1)
        t0 = torch.randint(0, hi, (batch_size,)) if starts is None else starts
        e = torch.randint(0, self.num_envs, (batch_size,)) if envs is None else envs
        return t0, e

    def _sample_torch(self, batch_size: int, starts=None, envs=None):
        """``sample`` by torch indexing: the CPU path, and what the device path is compared with and timed against."""
        t0, e = self._draw(batch_size, starts, envs)
        return _stack_torch(self.states, self.actions, self.rewards, self.dones, self.n_frames, batch_size, t0, e)

    def sample(self, batch_size: int, starts=None, envs=None):
        """Uniform sample of (turn, env) pairs with ``n_frames`` stacking:
        states, actions, rewards, next_states, dones, valid (``sorrel/buffers.py:98-124``).
        ``starts`` / ``envs`` override the random draws (first frame index and env of each sample).
        On a HIP device the batch is gathered by one ``sgw_sample`` launch into freshly allocated tensors.  There, indices the caller
        gives may name any row whose stacked frames lie inside the ring -- ``0 <= start < capacity - n_frames`` (not the size-based
        bound of the draws, ``max(1, size - n_frames - 1)``, which ``ReplaySampler`` also applies to given indices) and
        ``0 <= env < num_envs``: a host list outside that raises ``IndexError`` (negative entries do not wrap as they do under
        torch indexing on a CPU ring), a list whose length is not ``batch_size`` raises ``ValueError``; device tensors are passed
        through unchecked, and the kernel leaves the samples of indices outside those bounds unwritten."""
        if self.device.type != "cuda":
            return self._sample_torch(batch_size, starts, envs)
        t0, e = self._draw(batch_size, starts, envs)
        given = starts is not None or envs is not None
        # (the caller's own indices may name any row whose stacked frames lie inside the ring, as with torch indexing)
        return _sample_fresh(_ring_layout(self, None), self.n_frames, batch_size, t0, e,
                             self.capacity - self.n_frames if given else max(1, self.size - self.n_frames - 1))

    def returns(self, gamma: float, normalize=None, first=None, count=None, dtype=torch.float64, out=None) -> Returns:
        """Discounted returns of every env's stored turns, as the reference's PPO computes them at the head of ``train_step``
        (``sorrel/models/pytorch/ppo.py:226-239``): backwards in time, ``d = 0`` at every ``done``, ``d = reward + gamma * d`` in
        float32.  The segment defaults to everything stored, oldest to newest: rows ``0 .. size`` before the ring has wrapped,
        ``idx .. idx + capacity`` (mod ``capacity``) after; ``first`` / ``count`` name another one.  ``normalize="column"`` adds the
        reference's ``(x - mean) / (std + 1e-7)`` in float64 per env, ``"all"`` with one mean / std over the whole segment; ``dtype`` is
        the type the normalised values are stored in.  On a HIP device this is one ``sgw_returns`` call that reads the ring where it
        lies; with ``out=`` (an earlier result of the same shape and mode) it allocates nothing and does not synchronise, so it
        can be recorded into a graph."""
        return _ring_returns(self, None, gamma, normalize, first, count, dtype, out)

    def __repr__(self):
        return f"Buffer(capacity={self.capacity}, obs_shape={self.obs_shape}, num_envs={self.num_envs})"


class RolloutBuffer(Buffer):
    """The reference's ``RolloutBuffer`` (``sorrel/models/pytorch/ppo.py:21-65``) for all envs at once: a ``Buffer`` with a float32
    ``log_probs`` column ``[capacity, E]``, whose ``add`` takes the action as an ``(action, log_prob)`` pair.  ``returns()`` is what a
    policy-gradient learner opens its update with."""

    def __init__(self, capacity: int, obs_shape: Sequence[int], n_frames: int = 1, num_envs: int = 1, device=None, **extra):
        super().__init__(capacity, obs_shape, n_frames, num_envs, device, **extra)
        self.log_probs = torch.zeros((capacity, num_envs), dtype=torch.float32, device=self.device)

    def clear(self):
        super().clear()
        self.log_probs.zero_()

    def add(self, obs, action, reward, done, **extra):
        action_, log_prob = action
        # a recorded turn only counts (the engine's own kernels fill the row, by the device's row count: sgw_turn_policy_sample); and
        # log-probabilities the sampling launch has already written into this row are not copied again
        if not self._deferred:
            row = self.log_probs[self.idx]
            if not (torch.is_tensor(log_prob) and log_prob.dtype == torch.float32 and log_prob.data_ptr() == row.data_ptr()):
                self.log_probs[self.idx] = torch.as_tensor(log_prob, dtype=torch.float32, device=self.device)
        super().add(obs, action_, reward, done, **extra)


class SavedGames(Buffer):
    """The container ``generate_memories`` fills and writes (``sorrel/buffers.py:358-379``): a ``Buffer`` whose
    ``save`` also stores the extra columns (``positions``)."""

    def save(self, output_file) -> None:
        np.savez_compressed(Path(output_file), **self._file_arrays())

    def add_turns(self, states, actions, rewards, dones, **extra) -> None:
        """Append ``T`` turns at once from ``[T, E, ...]`` tensors (views of a ``TurnBuffer``); truncates at capacity
        like ``add_from_buffer``."""
        n = min(self.capacity - self.idx, states.shape[0])
        lo, hi = self.idx, self.idx + n
        self.states[lo:hi].copy_(states[:n].reshape((n,) + tuple(self.states.shape[1:])))
        self.actions[lo:hi].copy_(actions[:n])
        self.rewards[lo:hi].copy_(rewards[:n])
        self.dones[lo:hi].copy_(dones[:n])
        for key, value in extra.items():
            if value is not None and key in self.extra_data:
                self.extra_data[key][lo:hi].copy_(value[:n])
        self.idx = hi
        self.size = min(self.size + n, self.capacity)
        self._dones_dirty = True


class TurnBuffer:
    """Joint ring over ALL agents for fused rollouts: one slot holds one ``take_turn`` of every env --
    ``obs [capacity, E, A, *obs_shape]`` float32 (or uint8 for the compact format), ``actions`` uint8,
    ``rewards`` float32 ``[capacity, E, A]``.  ``Environment.collect`` points the step kernel's observation
    output at the slot, so the 617 MB of a config-3 turn are written once, by the kernel, where the learner reads
    them (the per-agent ``Buffer`` above gets a device-to-device copy per agent instead).  ``agent_view(a)``
    gives the reference's per-agent layout back as views."""

    def __init__(self, capacity: int, num_envs: int, obs_shape: Sequence[int], device=None, obs_dtype=torch.float32,
                 positions: bool = False):
        self.capacity, self.num_envs, self.obs_shape = capacity, num_envs, tuple(obs_shape)    # obs_shape = (A, C, V, V)
        self.device = resolve_device(device)
        A = self.obs_shape[0]
        self.obs = torch.zeros((capacity, num_envs, *self.obs_shape), dtype=obs_dtype, device=self.device)
        self.actions = torch.zeros((capacity, num_envs, A), dtype=torch.uint8, device=self.device)
        self.rewards = torch.zeros((capacity, num_envs, A), dtype=torch.float32, device=self.device)
        self.dones = torch.zeros((capacity, num_envs, A), dtype=torch.float32, device=self.device)   # all-zero inside an epoch
        # optional: every agent's (y, x) AFTER its move, what add_memory stores as ``positions`` (sorrel/agents/agent.py:127-130)
        self.positions = torch.zeros((capacity, num_envs, A, 2), dtype=torch.uint8, device=self.device) if positions else None
        self.idx = 0
        self.size = 0

    def slot(self) -> int:
        """The slot the next turn goes to (``commit`` advances)."""
        return self.idx

    def commit(self, actions: torch.Tensor, rewards: torch.Tensor, agent_pos: torch.Tensor = None) -> None:
        i = self.idx
        self.actions[i].copy_(actions)
        self.rewards[i].copy_(rewards)
        if self.positions is not None and agent_pos is not None:
            self.positions[i].copy_(agent_pos)
        self.idx = (self.idx + 1) % self.capacity
        self.size = min(self.size + 1, self.capacity)

    def advance(self, n: int) -> None:
        """``n`` consecutive slots starting at ``idx`` were filled in place (``Environment.collect`` through
        ``sgw_rollout``); the caller guarantees they do not wrap."""
        self.idx = (self.idx + n) % self.capacity
        self.size = min(self.size + n, self.capacity)

    def agent_view(self, a: int):
        """(states ``[capacity, E, C, V, V]``, actions, rewards, dones ``[capacity, E]``) of one agent slot: views."""
        return self.obs[:, :, a], self.actions[:, :, a], self.rewards[:, :, a], self.dones[:, :, a]

    def sample(self, batch_size: int, agent=None, n_frames: int = 1, starts=None, envs=None):
        """``Buffer.sample`` over the joint ring: states, actions (int64), rewards, next_states, dones, valid in the reference's
        shapes.  ``agent=a`` samples (turn, env) pairs of that agent; ``agent=None`` samples over every (env, agent) pair, for learners
        that share one model -- ``envs`` are then indices ``e * A + a``.  A CPU ring is read by torch indexing, a device ring by
        one ``sgw_sample`` launch, where it lies (uint8 observations widen to float32 on the way).  Drawn starts lie in
        ``[0, max(1, size - n_frames - 1))``; on a device ring given ones are checked as in ``Buffer.sample``:
        ``0 <= start < capacity - n_frames``, ``0 <= env < E`` (``E * A`` with ``agent=None``), ``IndexError`` for a host list."""
        E, A = self.num_envs, self.obs_shape[0]
        cols = E * A if agent is None else E
        hi = max(1, self.size - n_frames - 1)
        given = starts is not None or envs is not None
        t0 = torch.randint(0, hi, (batch_size,)) if starts is None else starts
        e = torch.randint(0, cols, (batch_size,)) if envs is None else envs
        if self.device.type == "cuda":
            return _sample_fresh(_ring_layout(self, agent), n_frames, batch_size, t0, e, self.capacity - n_frames if given else hi)
        if agent is None:
            tail = self.obs_shape[1:]
            st, ac = self.obs.reshape(self.capacity, cols, *tail), self.actions.reshape(self.capacity, cols)
            rw, dn = self.rewards.reshape(self.capacity, cols), self.dones.reshape(self.capacity, cols)
        else:
            if not 0 <= int(agent) < A:
                raise IndexError(f"agent {agent} outside [0, {A})")
            st, ac, rw, dn = self.agent_view(int(agent))
        s, a, r, ns, d, v = _stack_torch(st, ac, rw, dn, n_frames, batch_size, t0, e)
        return s.to(torch.float32), a.to(torch.int64), r, ns.to(torch.float32), d, v

    def returns(self, gamma: float, agent=None, normalize=None, first=None, count=None, dtype=torch.float64, out=None) -> Returns:
        """``Buffer.returns`` over the joint ring, read where it lies: ``agent=None`` runs over every (env, agent) column (``returns``
        ``[count, E, A]``, ``normalize="column"`` per env and agent), ``agent=a`` over that agent's columns (``[count, E]``)."""
        return _ring_returns(self, agent, gamma, normalize, first, count, dtype, out)

    def clear(self):
        self.idx = self.size = 0

    def __len__(self):
        return self.size


class ReplaySampler:
    """Training batches from a ``Buffer`` or a ``TurnBuffer`` on the device, one ``sgw_sample`` launch each, into storage this object
    owns: ``sample()`` returns the reference's six-tuple (states, actions, rewards, next_states, dones, valid) as views of that
    storage, valid until the next call.  With no indices given the kernel draws them itself from the counter RNG (stream
    ``STREAM_SAMPLE``, keyed by ``seed`` and a device-side call counter): no allocation, no copy to or from the host, no
    synchronisation, so a call can be recorded into a graph next to the turn and every replay draws a fresh batch.
    ``last_index`` ``[B, 2]`` holds the (start, env) pairs the last call used.  ``agent`` as in ``TurnBuffer.sample``.
    Given indices obey the bound of the draws, read from the ring at call time: ``0 <= start < max(1, size - n_frames - 1)``
    (tighter than ``Buffer.sample``'s ``capacity - n_frames`` for given indices: a sampler only hands out rows the ring has
    filled) and ``0 <= env <`` the ring's columns; host lists outside that raise ``IndexError``, a wrong length ``ValueError``,
    device tensors are passed through unchecked (the kernel leaves such samples unwritten)."""

    def __init__(self, ring, batch_size: int, *, n_frames=None, agent=None, seed: int = 0):
        self.ring, self.batch_size, self.agent, self.seed = ring, int(batch_size), agent, int(seed)
        self.n_frames = int(n_frames if n_frames is not None else getattr(ring, "n_frames", 1))
        if self.batch_size < 1 or self.n_frames < 1:
            raise ValueError("batch_size and n_frames must be at least 1")
        layout = _ring_layout(ring, agent)
        self.device = ring.device
        s, ns, a, r, d, v = _sample_outputs(self.batch_size, self.n_frames, layout["R"], self.device)
        for t in (s, ns, a, r, d, v):
            t.zero_()
        self._outs = (s, ns, a, r, d, v)
        self.last_index = torch.zeros((self.batch_size, 2), dtype=torch.int64, device=self.device)
        self.draw_count = torch.zeros((1,), dtype=torch.int64, device=self.device)     # (the kernel's uint64 counter)

    def num_starts(self) -> int:
        return max(1, self.ring.size - self.n_frames - 1)

    def max_starts(self) -> int:
        """``num_starts()`` of a full ring: the upper bound a clocked call hands to the kernel."""
        return max(1, self.ring.capacity - self.n_frames - 1)

    def batch(self):
        """The storage ``sample`` fills, in the order it returns it."""
        s, ns, a, r, d, v = self._outs
        return s, a, r, ns, d, v

    def sample(self, starts=None, envs=None, clock=None):
        """``clock``: the device address of an ``sgw_learn_clock`` whose ``num_starts`` the caller keeps at ``num_starts()``; the draws are then
        bounded by what the clock holds when the kernel runs (``sgw_sample_clocked``), which is what a recorded call needs while the ring fills."""
        if (starts is None) != (envs is None):
            raise ValueError("starts and envs are both given or both None")
        if clock is not None and (starts is not None or self.device.type != "cuda"):
            raise ValueError("clock= bounds indices drawn on the device: starts and envs must be None")
        layout = _ring_layout(self.ring, self.agent)
        hi, B = self.num_starts() if clock is None else self.max_starts(), self.batch_size
        if starts is not None:
            starts = _check_index_list("starts", starts, B, hi, self.device)
            envs = _check_index_list("envs", envs, B, layout["cols"], self.device)
        s, ns, a, r, d, v = self._outs
        if self.device.type != "cuda":
            if starts is None:
                raise RuntimeError("ReplaySampler draws its indices on the device: a CPU ring needs starts and envs")
            ring = self.ring
            if isinstance(ring, TurnBuffer):
                got = ring.sample(B, agent=self.agent, n_frames=self.n_frames, starts=starts, envs=envs)
            else:
                got = _stack_torch(ring.states, ring.actions, ring.rewards, ring.dones, self.n_frames, B, starts, envs)
            for dst, src in zip((s, a, r, ns, d, v), got):
                dst.copy_(src)
            self.last_index.copy_(torch.from_numpy(np.stack([starts, envs], axis=1)))
        else:
            if starts is not None:
                starts = torch.from_numpy(starts).to(self.device) if isinstance(starts, np.ndarray) else starts
                envs = torch.from_numpy(envs).to(self.device) if isinstance(envs, np.ndarray) else envs
            _launch_sample(layout, self.n_frames, B, self._outs, self.last_index, starts, envs, hi,
                           count=self.draw_count if starts is None else None, seed=self.seed, clock=clock)
        return self.batch()
