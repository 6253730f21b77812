"""GridEngine: owns the state tensors of E environments and drives the HIP kernels.

PyTorch is plumbing here (device memory, streams); all step/observe/reset
arithmetic runs in ``sorrel_amd/csrc/`` (``sgw.hip`` + the kernel headers it includes) through the C ABI of
``include/sgw.h``.  There is no CPU path: constructing an engine on a non-GPU
device raises.
"""
from __future__ import annotations

import ctypes as C
import functools
import itertools
import math
from typing import Optional

import torch

from . import _native as N
from ._check import check_tensor, refuse, tensor_ok
from .spec import WorldSpec, alloc_grid, resolve_device


def _index_vector(name, t, n: int, device) -> int:
    """The pointer of an int64 vector of which a kernel reads the first ``n`` entries."""
    if check_tensor(name, t, torch.int64, (...,), device).numel() < n:
        refuse(name, t, torch.int64, f"at least {n} elements", device)
    return t.data_ptr()


class GridEngine:
    """State + kernels for ``num_envs`` independent worlds on one GPU.

    Tensors (all on ``device``, per-env contiguous):
      grid ``uint8 [E,L,H,W]`` · agent_pos ``uint8 [E,A,2]`` · actions ``uint8 [E,A]``
      obs ``float32 [E,A,C,V,V]`` · rewards ``float32 [E,A]`` · total_reward ``float64 [E]``
    """

    def __init__(self, spec: WorldSpec, num_envs: int, device="cuda", first_env_id: int = 0,
                 allocate_obs: bool = True, tensors: Optional[dict] = None, obs_dtype=torch.float32):
        self.spec = spec
        self.num_envs = int(num_envs)
        self.first_env_id = int(first_env_id)
        self.device = resolve_device(device)
        if self.device.type != "cuda":
            raise N.SgwError(
                "GridEngine needs a HIP device (torch device 'cuda'); the step/observe path has no CPU fallback"
            )
        if not torch.cuda.is_available():
            raise N.SgwError("no HIP device visible to PyTorch; the step/observe path has no CPU fallback")
        self._dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self._lib = N.load()
        # every library call with a return code goes through N.call on the engine's device: self._call(self._lib.sgw_x, *args).  Bound
        # here (no Python frame of the engine's own per call); the caller's current stream on that device is self._stream(), an integer
        self._call = functools.partial(N.call, self._dev_index)
        self._stream = functools.partial(N.raw_stream, self._dev_index)
        self.uid = next(GridEngine._uids)        # names this engine in caches (id() values are reused once an object is gone)
        if GridEngine._pending_closes and not torch.cuda.is_current_stream_capturing():
            GridEngine.drain_pending_closes()    # (engines dropped inside an earlier capture: their handles are destroyed no later than here)
        E, A = self.num_envs, spec.num_agents
        dev = self.device
        tensors = tensors or {}
        # the grid may be a view with a padded env stride (spec.alloc_grid); inner dims must be dense
        g = tensors.get("grid")
        if g is None:
            g = alloc_grid(E, spec.layers, spec.height, spec.width, dev)
        hw = spec.height * spec.width
        if tuple(g.shape) != (E, spec.layers, spec.height, spec.width) or g.dtype != torch.uint8 or g.device != dev \
                or (E > 0 and tuple(g.stride()[1:]) != (hw, spec.width, 1)) or (E > 1 and g.stride(0) < spec.layers * hw):
            raise ValueError("grid must be uint8 [E, L, H, W] on the engine's device with dense (L, H, W) strides")
        self.grid = g
        self.config = spec.to_config(self.num_envs, self.first_env_id)
        cells = spec.layers * hw
        if E > 1:
            self.config.grid_env_stride = int(g.stride(0))
        else:   # one env: any stride is right; claim the padded one if the allocation really has the pad bytes
            pad = (cells + 15) // 16 * 16
            avail = g.untyped_storage().nbytes() - g.storage_offset()
            self.config.grid_env_stride = pad if avail >= pad else 0
        self._h = C.c_void_p()
        self._call(self._lib.sgw_create, C.byref(self.config), C.byref(self._h))

        def adopt(name, shape, dtype):
            t = tensors.get(name)
            return torch.zeros(shape, dtype=dtype, device=dev) if t is None else check_tensor(name, t, dtype, shape, dev)

        # state tensors may be adopted from the caller (the batched Gridworld owns them)
        self.agent_pos = adopt("agent_pos", (E, A, 2), torch.uint8)
        self.actions = adopt("actions", (E, A), torch.uint8)
        self.rewards = adopt("rewards", (E, A), torch.float32)
        self.total_reward = adopt("total_reward", (E,), torch.float64)
        self.metrics = torch.zeros((4,), dtype=torch.float64, device=dev)
        # float32 is the contract format (what the reference's replay buffer stores); uint8 is a compact
        # extra for one-hot specs (same layout, same values, 4x fewer bytes)
        if obs_dtype not in (torch.float32, torch.uint8):
            raise ValueError("obs_dtype must be torch.float32 or torch.uint8")
        self.obs_dtype = obs_dtype
        if obs_dtype == torch.uint8:
            self._call(self._lib.sgw_set_obs_format, self._h, N.OBS_U8)
        self.obs = (torch.zeros((E,) + spec.obs_shape, dtype=obs_dtype, device=dev) if allocate_obs else None)
        self.epoch = 0
        self.turn = 0
        self.row_tail = 0               # elements bind_row_tail appends behind every window of a row
        self._tail_table = None
        self._scratch_obs = None
        self.max_turns = 0              # set_auto_reset: epoch length (0 = no auto-reset)
        self.episode_return = None      # [E] float64: total_reward of the epoch that just ended
        # per-env agent state (current entity type of each agent): needed by interaction rules (Tag)
        self.agent_state = self.state_at_pov = None
        if spec.agent_rule == N.AGENT_RULE_TAG:
            self.agent_state = adopt("agent_state", (E, A), torch.uint8)
            self.state_at_pov = torch.zeros((E, A), dtype=torch.uint8, device=dev)
            self._call(self._lib.sgw_bind_agent_state, self._h, self.agent_state.data_ptr(), self.state_at_pov.data_ptr())
            if "agent_state" not in tensors:
                self._call(self._lib.sgw_init_agent_state, self._h, self.agent_state.data_ptr(), self._stream())
        # per-env facing of each agent, 0 up / 1 right / 2 down / 3 left (Cleanup's beams)
        self.agent_dir = None
        if spec.agent_rule == N.AGENT_RULE_CLEANUP:
            self.agent_dir = tensors.get("agent_dir")
            if self.agent_dir is None:
                self.agent_dir = torch.full((E, A), 2, dtype=torch.uint8, device=dev)   # CleanupAgent.__init__: facing down (agents.py:74); like Tag's flag it survives resets
            check_tensor("agent_dir", self.agent_dir, torch.uint8, (E, A), dev)
            self._call(self._lib.sgw_bind_agent_dir, self._h, self.agent_dir.data_ptr())

        # what every agent stepped on this turn (uint8 [E, A]; N.NO_TARGET: invalid action / outside the grid): on request only
        self.target_types = None
        if tensors.get("target_types") is not None:
            self.bind_target_types(tensors["target_types"])
        # what the agents found, summed (int64 [E, A, K]): on request only -- (slot_of_type, K, counts)
        self.encounters = None
        if tensors.get("encounters") is not None:
            self.bind_encounters(*tensors["encounters"])

    def bind_target_types(self, t=True):
        """``sgw_bind_target_types``: from now on every act of a plain mover records the entity type it found on its target cell in
        ``self.target_types`` (uint8 ``[E, A]``; ``N.NO_TARGET`` for an invalid action or a target outside the grid) -- what
        ``GamblingAgent.act`` counts as an encounter.  ``t``: True allocates the tensor, a tensor adopts it, None / False unbinds."""
        E, A = self.num_envs, self.spec.num_agents
        if t is None or t is False:
            self._call(self._lib.sgw_bind_target_types, self._h, None)
            self.target_types = None
            return None
        if t is True:
            t = self.target_types if self.target_types is not None else torch.full((E, A), N.NO_TARGET, dtype=torch.uint8, device=self.device)
        check_tensor("target_types", t, torch.uint8, (E, A), self.device)
        self._call(self._lib.sgw_bind_target_types, self._h, t.data_ptr())
        self.target_types = t
        return t

    def bind_encounters(self, slot_of_type, num_slots=None, counts=None):
        """``sgw_bind_encounters``: from now on every act of a plain mover or a Cleanup agent adds what it found on its target cell to
        ``self.encounters`` (int64 ``[E, A, num_slots]``): plain movers the type on the agent layer, Cleanup agents the type on every layer.
        ``slot_of_type``: one entry per entity type of the spec, the slot the type counts in or ``N.NO_SLOT``; None unbinds.  ``counts``
        adopts a tensor (it is not zeroed: the library never clears the counts, the caller decides when), default a zeroed one.
        ``ValueError`` for what the library refuses: Tag agents, a slot outside ``[0, num_slots)``, ``num_slots`` outside 1..32."""
        if slot_of_type is None:
            self._call(self._lib.sgw_bind_encounters, self._h, None, None, 0)
            self.encounters = None
            return None
        E, A, T = self.num_envs, self.spec.num_agents, int(self.config.num_types)
        slots = [int(s) for s in slot_of_type]
        if len(slots) != T:
            raise ValueError(f"slot_of_type needs one entry per entity type: {T}, not {len(slots)}")
        if any(s < 0 or s > 255 for s in slots):
            raise ValueError("slot_of_type entries are slot numbers or N.NO_SLOT (255)")
        if num_slots is None:
            num_slots = max([s + 1 for s in slots if s != N.NO_SLOT], default=0)
        K = int(num_slots)
        if not 1 <= K <= 32:
            raise ValueError(f"num_slots must be in 1..32, not {K}")
        if counts is None:
            counts = torch.zeros((E, A, K), dtype=torch.int64, device=self.device)
        check_tensor("counts", counts, torch.int64, (E, A, K), self.device)
        table = (C.c_uint8 * T)(*slots)
        self._call(self._lib.sgw_bind_encounters, self._h, counts.data_ptr(), C.cast(table, C.c_void_p), K)
        self.encounters = counts
        return counts

    # ------------------------------------------------------------------ util
    def _on_device(self):
        """Context that makes the engine's device current for as long as a caller wants to hold it (``_FastPolicyTurn``: across the
        agents' forward passes); a single call needs none, ``self._call`` sees to the device itself."""
        return N.on_device(self._dev_index)

    @property
    def window_shape(self) -> tuple:
        """``(E, C, V, V)``: one agent's window in every env."""
        return (self.num_envs,) + tuple(self.spec.obs_shape[1:])

    @property
    def window_elems(self) -> int:
        """``C * V * V``: the elements of one window (a replay row holds that many, plus ``row_tail``)."""
        return math.prod(self.window_shape[1:])

    def is_window_rows(self, t, tail: int = 0) -> bool:
        """Whether ``t`` is one window (+ ``tail`` elements) per env as the kernels write it (``SGW_STEP_OBS_NEXT_PACKED``, the row
        kernels): ``E`` contiguous rows of exactly ``C*V*V + tail`` elements of the engine's observation dtype on its device, whatever
        the trailing shape (``[E, C, V, V]`` or a replay row ``[E, C*V*V]``)."""
        return tensor_ok(t, self.obs_dtype, (self.num_envs, None, ...), self.device) \
            and t.numel() == self.num_envs * (self.window_elems + tail)

    def _check_obs(self, t: torch.Tensor, name: str) -> torch.Tensor:
        """An observation destination: exactly the ``E * A * C * V * V`` elements the step kernel writes."""
        return check_tensor(name, t, self.obs_dtype, (self.num_envs,) + tuple(self.spec.obs_shape), self.device)

    def _check_window(self, t: torch.Tensor, name: str, tail: int = 0) -> torch.Tensor:
        if not self.is_window_rows(t, tail):
            refuse(name, t, self.obs_dtype, f"{self.num_envs} rows of {self.window_elems + tail} elements", self.device)
        return t

    def _check_pos(self, t: torch.Tensor) -> torch.Tensor:
        return check_tensor("pos", t, torch.uint8, (self.num_envs, self.spec.num_agents, 2), self.device)

    _pending_closes: list = []        # (library, handle) of engines dropped while a stream was capturing: destroyed by drain_pending_closes()
    _uids = itertools.count(1)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            h, self._h = self._h, C.c_void_p()
            # sgw_destroy frees device memory, which HIP forbids while a stream of the process is capturing (the capture fails and torch
            # aborts while it unwinds): an engine that dies inside a capture -- the collector's doing or a plain refcount -- waits
            try:
                capturing = torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()
            except Exception:
                capturing = False
            if capturing:
                GridEngine._pending_closes.append((self._lib, h))
            else:
                self._lib.sgw_destroy(h)             # (not through _call, here and below: it returns nothing, and may run at interpreter shutdown)

    @classmethod
    def drain_pending_closes(cls) -> int:
        """Destroy the engines whose ``close()`` came while a stream was capturing.  Called before and after ``capture_turn``'s capture."""
        n = 0
        while cls._pending_closes:
            lib, h = cls._pending_closes.pop()
            lib.sgw_destroy(h)
            n += 1
        return n

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ ops
    def reset(self, epoch: Optional[int] = None):
        """create_world + populate_environment for every env (K3)."""
        if epoch is not None:
            self.epoch = int(epoch)
        self.turn = 0
        self._call(self._lib.sgw_reset, self._h, self.grid.data_ptr(), self.agent_pos.data_ptr(), self.total_reward.data_ptr(),
                   self.epoch, self._stream())

    def observe(self, agent_begin: int = 0, agent_end: Optional[int] = None, out: Optional[torch.Tensor] = None,
                pos: Optional[torch.Tensor] = None):
        """Stateless egocentric observation of the agents (K1).  ``pos`` (uint8 ``[E, A, 2]``)
        observes from other cells than the agents' own."""
        out = self.obs if out is None else self._check_obs(out, "out")
        if out is None:
            raise ValueError("engine was built with allocate_obs=False; pass `out`")
        pos = self.agent_pos if pos is None else self._check_pos(pos)
        agent_end = self.spec.num_agents if agent_end is None else agent_end
        self._call(self._lib.sgw_observe, self._h, self.grid.data_ptr(), pos.data_ptr(), out.data_ptr(), agent_begin, agent_end, self._stream())
        return out

    # ------------------------------------------------------------------ policy-driven turns without re-rendering
    def capabilities(self) -> int:
        """``N.CAP_OBSERVE_ROWS`` | ``N.CAP_ACT`` (include/sgw.h)."""
        return int(self._lib.sgw_capabilities(self._h))       # (not through _call: the return value is the capability mask)

    def window_rows(self, dests=None):
        """The per-agent window destinations ``sgw_observe_rows`` / ``sgw_act`` take: ``(ctypes pointer array, env stride in
        elements, the tensors)``.  ``dests`` = one tensor per agent, each ``num_envs`` contiguous rows of exactly one window
        (``C*V*V`` elements of the engine's observation dtype, e.g. a row of that agent's replay buffer); default = the
        slots of the observation tensor ``self.obs[:, a]``."""
        A, per_env = self.spec.num_agents, self.window_elems
        arr = (C.c_void_p * A)()
        if dests is None:
            if self.obs is None:
                raise ValueError("engine was built with allocate_obs=False; pass per-agent destinations")
            base, esz = self.obs.data_ptr(), self.obs.element_size()
            for a in range(A):
                arr[a] = base + a * per_env * esz
            return arr, A * per_env, None
        if len(dests) != A:
            raise ValueError(f"need one destination per agent ({A}), got {len(dests)}")
        for a, t in enumerate(dests):
            arr[a] = self._check_window(t, f"dests[{a}]", self.row_tail).data_ptr()
        return arr, per_env + self.row_tail, list(dests)

    def sweep_observe_rows(self, rows, sweep: bool = True, turn: Optional[int] = None):
        """Steps 1 and 2 of a policy-driven turn in ONE launch (``sgw_sweep_observe_rows``, ``CAP_SWEEP_ROWS``): the entity sweep, then every
        agent's window of the swept grid into its own destination (``rows`` from ``window_rows``, exactly one window per env and row)."""
        arr, stride, _ = rows
        turn = self.turn if turn is None else turn
        self._call(self._lib.sgw_sweep_observe_rows, self._h, self.grid.data_ptr(), self.agent_pos.data_ptr(), arr, stride, self.epoch, turn,
                   N.STEP_SWEEP if sweep else 0, self._stream())

    def observe_rows(self, rows, agent_begin: int = 0, agent_end: Optional[int] = None):
        """Every agent's window, once, into its own destination (``rows`` from ``window_rows``): step 2 of a policy-driven
        turn.  Needs ``CAP_OBSERVE_ROWS``; otherwise ``observe()`` into the observation tensor does the same job."""
        arr, stride, _ = rows
        agent_end = self.spec.num_agents if agent_end is None else agent_end
        self._call(self._lib.sgw_observe_rows, self._h, self.grid.data_ptr(), self.agent_pos.data_ptr(), arr, stride,
                   agent_begin, agent_end, self._stream())

    _ACTION_KINDS = {torch.uint8: N.ACT_U8, torch.int32: N.ACT_I32, torch.int64: N.ACT_I64}

    def is_action_values(self, action) -> bool:
        """A policy's VALUE output -- float32 ``[E, n_actions]`` -- which ``act`` / ``turn_act`` take as it is (``SGW_ACT_QF32``: the
        kernel picks the first index of each row's maximum, and explores by ``turn_epsilon`` under the turn protocol)."""
        return tensor_ok(action, torch.float32, (self.num_envs, self.spec.num_actions), self.device)

    def is_direct_action(self, action) -> bool:
        """Whether the act launches take ``action`` as it is: ``[E]`` uint8 / int32 / int64, contiguous, on the device (a policy's output
        needs no narrowing copy), or action values (``is_action_values``).  Anything else is copied into ``self.actions`` first."""
        if not torch.is_tensor(action):
            return False
        if action.dtype in self._ACTION_KINDS:
            return tensor_ok(action, action.dtype, (self.num_envs,), self.device)
        return self.is_action_values(action)

    def _action_arg(self, action):
        """(pointer, SGW_ACT_* kind) of a caller's action tensor, which must be a direct one (``is_direct_action``); ``None``: ``(0, 0)``."""
        if action is None:
            return 0, 0
        if not self.is_direct_action(action):
            refuse("action", action, "uint8 / int32 / int64", f"shape [{self.num_envs}] -- or float32 action values "
                   f"[{self.num_envs}, {self.spec.num_actions}] --", self.device)
        return action.data_ptr(), self._ACTION_KINDS.get(action.dtype, N.ACT_QF32)

    def act(self, agent: int, rows=None, action: Optional[torch.Tensor] = None, reward_row: Optional[torch.Tensor] = None,
            action_row: Optional[torch.Tensor] = None):
        """``MovingAgent.act`` of ONE agent for every env; the at most two cells the move changes are rewritten in the
        windows (``rows``) of the agents after it that contain them, so that each later agent's window shows the grid after
        the moves of all agents before it, without being rendered again.  The agent's actions are ``self.actions[:, agent]``
        or, with ``action``, that ``[E]`` tensor as it is (uint8 / int32 / int64, contiguous, on the device: a policy's
        output needs no narrowing copy; ``self.actions[:, agent]`` still records what was taken).  Rewards land in
        ``self.rewards[:, agent]`` and, with ``reward_row`` (float32 ``[E]``) / ``action_row`` (int64 ``[E]``), a second
        time in those rows -- e.g. the rows of the agent's replay buffer."""
        arr, stride = (None, 0) if rows is None else (rows[0], rows[1])
        E, dev = self.num_envs, self.device
        pa, kind = self._action_arg(action)
        prr = None if reward_row is None else check_tensor("reward_row", reward_row, torch.float32, E, dev).data_ptr()
        par = None if action_row is None else check_tensor("action_row", action_row, torch.int64, E, dev).data_ptr()
        self._call(self._lib.sgw_act, self._h, self.grid.data_ptr(), self.agent_pos.data_ptr(), self.actions.data_ptr(), arr, stride,
                   self.rewards.data_ptr(), self.total_reward.data_ptr(), int(agent), pa or None, kind, prr, par, self._stream())
        return self.rewards[:, agent] if reward_row is None else reward_row

    def bind_row_tail(self, kind: int, table: Optional[torch.Tensor] = None):
        """``sgw_bind_row_tail``: what the agents' ``pov`` appends behind the flattened window, written by ``observe_rows`` (and kept
        current by ``act``) instead of a ``torch.cat`` on the host: ``N.TAIL_AGENT_IS_IT`` (Tag: one element) or
        ``N.TAIL_POSITION_TABLE`` with ``table`` float32 ``[H, W, tail_len]`` on the device (Cleanup's positional code).  Rows passed
        to ``window_rows`` then hold ``C*V*V + tail`` elements per env."""
        n = 0
        if kind == N.TAIL_POSITION_TABLE:
            n = int(check_tensor("table", table, torch.float32, (self.spec.height, self.spec.width, None), self.device).shape[2])
        elif kind == N.TAIL_AGENT_IS_IT:
            n = 1
        if self.obs_dtype != torch.float32 and kind != N.TAIL_NONE:
            raise ValueError("row tails are float32 (the observation format must be float32)")
        self._call(self._lib.sgw_bind_row_tail, self._h, int(kind), n, table.data_ptr() if kind == N.TAIL_POSITION_TABLE else None)
        self.row_tail, self._tail_table = n, table

    # ------------------------------------------------------------------ a whole policy turn as one capturable submission
    def turn_bind(self, rings=None):
        """``sgw_turn_bind``: the agents' replay rings -- one ``(states, rewards, actions, dones, row, step)`` per agent (or ``None``
        for an agent that keeps no replay rows): ``states [capacity, E, >= C*V*V]`` of the engine's observation dtype, ``rewards``
        float32 / ``actions`` int64 / ``dones`` float32 ``[capacity, E]`` (each may be ``None``; ``dones`` is zeroed for the turn's
        row), ``row`` = the ring row the NEXT turn fills, ``step`` = rows the ring advances per turn.  ``rings=None`` unbinds.
        Blocking; not for the inside of a capture."""
        A, E = self.spec.num_agents, self.num_envs
        self._turn_rings, self._turn_row_elems = None, [0] * A
        if rings is None:
            self._call(self._lib.sgw_turn_bind, self._h, None)
            return
        if len(rings) != A:
            raise ValueError(f"need one ring (or None) per agent ({A}), got {len(rings)}")
        rows = N.SgwTurnRows()
        keep = []
        for a, ring in enumerate(rings):
            if ring is None:
                continue
            states, rewards, actions, dones, row, step = ring
            cap = None
            for name, t, dt, size in (("states", states, self.obs_dtype, (None, E, ...)), ("rewards", rewards, torch.float32, (None, E)),
                                      ("actions", actions, torch.int64, (None, E)), ("dones", dones, torch.float32, (None, E))):
                if t is None:
                    continue
                check_tensor(f"rings[{a}].{name}", t, dt, size, self.device)
                if cap is not None and t.shape[0] != cap:
                    raise ValueError(f"rings[{a}]: states / rewards / actions disagree on the capacity")
                cap = int(t.shape[0])
            if cap is None:
                continue
            if states is not None:
                rows.states[a] = states.data_ptr()
                rows.row_elems[a] = self._turn_row_elems[a] = states[0, 0].numel()      # (turn_prev_rows writes rows of that length)
            if rewards is not None:
                rows.rewards[a] = rewards.data_ptr()
            if actions is not None:
                rows.actions[a] = actions.data_ptr()
            if dones is not None:
                rows.dones[a] = dones.data_ptr()
            rows.capacity[a], rows.row[a], rows.step[a] = cap, int(row), int(step)
            keep.append((states, rewards, actions, dones))
        self._turn_rings = keep            # (the device state holds raw pointers into these)
        self._call(self._lib.sgw_turn_bind, self._h, C.byref(rows))

    def turn_set(self, epoch: Optional[int] = None, turn: Optional[int] = None):
        """``sgw_turn_set``: the turn the device has counted up to (stream-ordered; ``Environment.reset`` -> ``(epoch, 0)``)."""
        self._call(self._lib.sgw_turn_set, self._h, self.epoch if epoch is None else int(epoch), self.turn if turn is None else int(turn),
                   self._stream())

    def turn_begin(self, sweep: bool = True):
        """``sgw_turn_begin``: ``turn += 1`` on the device, then the sweep and EVERY agent's window into ``self.obs``."""
        if self.obs is None:
            raise ValueError("turn_begin needs the observation tensor (allocate_obs=True)")
        self._call(self._lib.sgw_turn_begin, self._h, self.grid.data_ptr(), self.agent_pos.data_ptr(), self.actions.data_ptr(), self.obs.data_ptr(),
                   self.rewards.data_ptr(), self.total_reward.data_ptr(), N.STEP_SWEEP if sweep else 0, self._stream())
        return self.obs

    def turn_act(self, agent: int, action: Optional[torch.Tensor] = None):
        """``sgw_turn_act``: ``act`` of one agent with the windows in ``self.obs``; reward and int64 action also go to the agent's ring
        row of the turn in flight (by the device's own row count)."""
        pa, kind = self._action_arg(action)
        self._call(self._lib.sgw_turn_act, self._h, self.grid.data_ptr(), self.agent_pos.data_ptr(), self.actions.data_ptr(), self.obs.data_ptr(),
                   self.rewards.data_ptr(), self.total_reward.data_ptr(), int(agent), pa or None, kind, self._stream())
        return self.rewards[:, agent]

    def turn_begin_rows(self, rows, sweep: bool = True):
        """``sgw_turn_begin_rows``: the sweep alone, then every agent's window into its row of ``rows`` (``window_rows(dests)``) AND -- by
        the device's row count -- into its replay row of the turn in flight."""
        arr, stride, _ = rows
        self._call(self._lib.sgw_turn_begin_rows, self._h, self.grid.data_ptr(), self.agent_pos.data_ptr(), self.actions.data_ptr(),
                   self.rewards.data_ptr(), self.total_reward.data_ptr(), arr, stride, N.STEP_SWEEP if sweep else 0, self._stream())

    def turn_act_rows(self, agent: int, rows, action: Optional[torch.Tensor] = None):
        """``sgw_turn_act_rows``: ``act`` of one agent, the repairs written to the later agents' rows of ``rows`` and to their replay rows."""
        arr, stride, _ = rows
        pa, kind = self._action_arg(action)
        self._call(self._lib.sgw_turn_act_rows, self._h, self.grid.data_ptr(), self.agent_pos.data_ptr(), self.actions.data_ptr(), arr, stride,
                   self.rewards.data_ptr(), self.total_reward.data_ptr(), int(agent), pa or None, kind, self._stream())
        return self.rewards[:, agent]

    def turn_end(self, commit_windows: bool = True):
        """``sgw_turn_end``: the turn's windows -> the agents' ring rows, every ring advances."""
        self._call(self._lib.sgw_turn_end, self._h, self.obs.data_ptr() if (commit_windows and self.obs is not None) else None, self._stream())

    # ------------------------------------------------------------------ stochastic policies
    def _policy_dist(self, dist):
        """(tensor, SGW_POLICY_* dist type, mode) of an ``ActionProbs`` / ``ActionLogits`` -- or of a bare tensor, taken as probabilities."""
        from sorrel_amd.models.base_model import ActionProbs

        t, logits = (dist.tensor, dist.logits) if isinstance(dist, ActionProbs) else (dist, False)
        if not torch.is_tensor(t) or t.dim() != 2 or t.dtype not in (torch.float32, torch.float64) or t.device != self.device \
                or t.stride(1) != 1 or t.stride(0) < t.shape[1] or not 1 <= t.shape[1] <= N.POLICY_MAX_ACTIONS:
            got = (tuple(t.shape), t.dtype, t.device) if torch.is_tensor(t) else type(t)
            raise ValueError(f"a distribution is a float32 / float64 [n, 1..{N.POLICY_MAX_ACTIONS}] tensor on {self.device} whose rows are contiguous (got {got})")
        return t, (N.POLICY_F64 if t.dtype == torch.float64 else N.POLICY_F32), (N.POLICY_LOGITS if logits else N.POLICY_PROBS)

    def _policy_out(self, t, n, dtype, name):
        return None if t is None else check_tensor(name, t, dtype, n, self.device)

    def policy_sample(self, dist, agent: int = 0, idx: Optional[torch.Tensor] = None, epoch: Optional[int] = None, turn: Optional[int] = None,
                      out_actions: Optional[torch.Tensor] = None, out_log_probs: Optional[torch.Tensor] = None,
                      out_entropy: Optional[torch.Tensor] = None):
        """``sgw_policy_sample``: one action per row of ``dist`` (``ActionProbs`` / ``ActionLogits``, or a bare tensor of probabilities;
        ``[n, n_actions]``), its log-probability and the row's entropy -- ``Categorical(...).sample()`` / ``.log_prob()`` / ``.entropy()``
        with the draw keyed by (seed, env, ``epoch``, ``turn``, agent) instead of consumed from a generator.  Row ``k`` belongs to
        (env, agent) = ``(k % E, agent + k // E)`` -- one agent's ``[E]`` rows, a shared model's agent-major ``[A * E]`` rows -- or, with
        ``idx`` (int64 ``[n]``), to ``(idx[k] % E, idx[k] // E)``.  ``epoch`` / ``turn`` default to the engine's (the turn in flight).
        Returns ``(actions int64 [n], log_probs float32 [n], entropy float32 [n])``; with all three ``out_*`` given the call allocates
        nothing and does not synchronise.  ``out_log_probs=False`` / ``out_entropy=False``: not wanted (not computed; None is returned)."""
        t, dtype, mode = self._policy_dist(dist)
        n = int(t.shape[0])
        self._policy_out(idx, n, torch.int64, "idx")
        acts = self._policy_out(out_actions, n, torch.int64, "out_actions")
        lps = None if out_log_probs is False else self._policy_out(out_log_probs, n, torch.float32, "out_log_probs")
        ents = None if out_entropy is False else self._policy_out(out_entropy, n, torch.float32, "out_entropy")
        if acts is None:
            acts = torch.empty((n,), dtype=torch.int64, device=self.device)
        if lps is None and out_log_probs is not False:
            lps = torch.empty((n,), dtype=torch.float32, device=self.device)
        if ents is None and out_entropy is not False:
            ents = torch.empty((n,), dtype=torch.float32, device=self.device)
        if n == 0:
            return acts, lps, ents
        d = N.SgwPolicyDesc()
        d.dist, d.idx = t.data_ptr(), (idx.data_ptr() if idx is not None else None)
        d.out_actions = acts.data_ptr()
        d.out_log_probs, d.out_entropy = (lps.data_ptr() if lps is not None else None), (ents.data_ptr() if ents is not None else None)
        d.n, d.num_envs, d.row_stride, d.num_actions = n, self.num_envs, int(t.stride(0)) if n > 1 else int(t.shape[1]), int(t.shape[1])
        d.seed, d.first_env = int(self.spec.seed) & 0xFFFFFFFFFFFFFFFF, self.first_env_id
        d.epoch, d.turn = int(self.epoch if epoch is None else epoch), int(self.turn if turn is None else turn)
        d.agent0, d.dist_type, d.mode = int(agent), dtype, mode
        N.launch("sgw_policy_sample", d, self.device)
        return acts, lps, ents

    def turn_policy_sample(self, agent: int, dist, out_actions: torch.Tensor, log_prob_ring: Optional[torch.Tensor] = None,
                           out_entropy: Optional[torch.Tensor] = None):
        """``sgw_turn_policy_sample``: agent ``agent``'s ``[E, n_actions]`` distribution sampled under the turn protocol -- epoch, the turn in
        flight and the row of ``log_prob_ring`` (float32 ``[capacity, E]``: a ``RolloutBuffer``'s ``log_probs``) that receives the
        log-probabilities are the device's own count, so the call is the same every turn and can be recorded.  ``out_actions`` int64 ``[E]``
        is what ``turn_act`` then takes."""
        t, dtype, mode = self._policy_dist(dist)
        E = self.num_envs
        if tuple(t.shape) != (E, self.spec.num_actions) or not t.is_contiguous():
            raise ValueError(f"the distribution of a turn is a contiguous [{E}, {self.spec.num_actions}] tensor; got {tuple(t.shape)}")
        acts = self._policy_out(out_actions, E, torch.int64, "out_actions")
        if acts is None:
            raise ValueError("turn_policy_sample writes its actions to out_actions (a fixed address a recorded turn can replay)")
        ents = self._policy_out(out_entropy, E, torch.float32, "out_entropy")
        ring = None if log_prob_ring is None else check_tensor("log_prob_ring", log_prob_ring, torch.float32, (None, E), self.device)
        self._call(self._lib.sgw_turn_policy_sample, self._h, int(agent), t.data_ptr(), dtype, mode, acts.data_ptr(),
                   ring.data_ptr() if ring is not None else None, ents.data_ptr() if ents is not None else None, self._stream())
        return acts

    # ------------------------------------------------------------------ speculative policy turns
    def speculation_rows(self, rows: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``[A, E, C*V*V]`` float32, agent-major: the windows the policies read in a speculative turn (``turn_resolve``).  Agents that
        share a model are one contiguous ``[A_g * E, C*V*V]`` batch of it.  ``rows``: the caller's own tensor of that shape -- e.g. the
        ``A`` rows of a shared replay ring this turn fills -- instead of the engine's scratch."""
        A, E, per_env = self.spec.num_agents, self.num_envs, self.window_elems
        if getattr(self, "_spec_state", None) is None:
            self._spec_state = torch.zeros((4, E, A), dtype=torch.uint8, device=self.device)      # env_done (the first E bytes of [0]), pristine, dirty, previous moves
            self._spec_list = torch.zeros((2, E * A), dtype=torch.int64, device=self.device)      # the dirty rows of the odd / even passes
            self._spec_ctr = torch.zeros((8,), dtype=torch.int32, device=self.device)             # ... and how many (pass & 7)
            self._spec_rows = None
            self._spec_cache = {}
        if rows is None:
            if self._spec_rows is None:
                self._spec_rows = torch.zeros((A, E, per_env), dtype=torch.float32, device=self.device)
            return self._spec_rows
        return check_tensor("rows", rows, torch.float32, (A, E, per_env), self.device)

    def gather_rows(self, flat: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
        """``flat[idx]`` for float32 rows (``sgw_gather_rows``: the dirty rows of a speculative pass as one contiguous batch) into a buffer
        the engine keeps; valid until the next call."""
        check_tensor("flat", flat, torch.float32, (None, None), self.device)
        check_tensor("idx", idx, torch.int64, (..., ), self.device)
        n, ne = int(idx.numel()), int(flat.shape[1])
        buf = getattr(self, "_gather_buf", None)
        if buf is None or buf.shape[1] != ne or buf.shape[0] < n:
            buf = self._gather_buf = torch.empty((max(n, 4096), ne), dtype=torch.float32, device=self.device)
        self._call(self._lib.sgw_gather_rows, flat.data_ptr(), ne, idx.data_ptr(), n, buf.data_ptr(), self._stream())
        return buf[:n]

    def choose_actions(self, values: torch.Tensor, idx: Optional[torch.Tensor], epoch: int, turn: int) -> torch.Tensor:
        """``sgw_choose_actions``: the actions ``sgw_act`` would take from these action values ``[n, num_actions]`` (row k belongs to the
        (agent, env) pair ``idx[k] = agent * E + env``; ``idx`` None: ``k`` itself) -- argmax, or with probability epsilon[agent]
        (``turn_epsilon``) the engine's keyed draw for (env, ``turn``, agent).  int64 ``[n]``."""
        n = int(values.shape[0])
        if values.dim() != 2 or values.shape[1] != self.spec.num_actions or not values.is_floating_point():
            raise ValueError(f"action values must be floating point [n, {self.spec.num_actions}]; got {values.dtype} {tuple(values.shape)}")
        values = values.to(device=self.device, dtype=torch.float32).contiguous()
        out = torch.empty((n,), dtype=torch.int64, device=self.device)
        self._call(self._lib.sgw_choose_actions, self._h, values.data_ptr(), None if idx is None else _index_vector("idx", idx, n, self.device),
                   n, int(epoch), int(turn), out.data_ptr(), self._stream())
        return out

    def verify_rows(self, played: "GridEngine", rows: torch.Tensor) -> None:
        """``sgw_verify_rows``: ``played`` is a scratch engine that has just played this turn's current actions as ONE sequential turn
        (``step(actions, sweep=False)``: its ``obs`` are the windows the agents really had, its ``state_at_pov`` Tag's flags); every row of
        ``rows`` ``[A, E, C*V*V + tail]`` that differs is rewritten and listed (``verify_count`` / ``verify_list``)."""
        A, E = self.spec.num_agents, self.num_envs
        check_tensor("rows", rows, torch.float32, (A, E, None), self.device)
        self._check_obs(played.obs, "played.obs")            # (the kernel reads this engine's E * A windows there)
        flags = None
        if self.spec.agent_rule == N.AGENT_RULE_TAG:
            flags = check_tensor("played.state_at_pov", played.state_at_pov, torch.uint8, (E, A), self.device).data_ptr()
        if getattr(self, "_verify_list", None) is None:
            self._verify_list = torch.zeros((E * A,), dtype=torch.int64, device=self.device)
            self._verify_ctr = torch.zeros((1,), dtype=torch.int32, device=self.device)
        self._call(self._lib.sgw_verify_rows, self._h, played.obs.data_ptr(), flags, rows.data_ptr(), int(rows.shape[2]),
                   self._verify_list.data_ptr(), self._verify_ctr.data_ptr(), self._stream())

    def verify_count(self) -> int:
        """How many rows the last ``verify_rows`` rewrote (synchronises: the one read-back per pass)."""
        return int(self._verify_ctr.item())

    def apply_actions(self, idx: Optional[torch.Tensor], fresh: torch.Tensor, n: int) -> None:
        """``sgw_apply_actions``: ``actions[e, a] = fresh[k]`` for the k-th row index ``a * E + e`` of ``idx`` (None: k itself), k < n."""
        n = int(n)
        self._call(self._lib.sgw_apply_actions, self._h, self.actions.data_ptr(), None if idx is None else _index_vector("idx", idx, n, self.device),
                   _index_vector("fresh", fresh, n, self.device), n, self._stream())

    def speculation_windows(self, rows: Optional[torch.Tensor] = None, sweep_turn: Optional[int] = None) -> torch.Tensor:
        """Every agent's PRE-move window into ``speculation_rows(rows)``: ``sgw_observe_rows`` where the engine has a row kernel for the
        world (one-hot tables), else ``sgw_turn_resolve``'s render mode (any table).  ``sweep_turn``: the entity sweep of that turn runs
        first -- in the same launch where the engine has ``CAP_SWEEP_ROWS``."""
        rows = self.speculation_rows(rows)
        caps = self.capabilities()
        if caps & N.CAP_OBSERVE_ROWS and not self.row_tail:
            key = rows.data_ptr()
            wr = self._spec_cache.get(key)
            if wr is None:
                if len(self._spec_cache) > 64:
                    self._spec_cache.clear()
                wr = self._spec_cache[key] = self.window_rows([rows[a] for a in range(self.spec.num_agents)])
            if sweep_turn is not None and caps & N.CAP_SWEEP_ROWS:
                self.sweep_observe_rows(wr, sweep=True, turn=sweep_turn)
                return rows
            if sweep_turn is not None:
                self.step(self.actions, sweep=True, agent_begin=0, agent_end=0, write_obs=False, turn=sweep_turn)
            self.observe_rows(wr)
        else:
            if sweep_turn is not None:
                self.step(self.actions, sweep=True, agent_begin=0, agent_end=0, write_obs=False, turn=sweep_turn)
            self.turn_resolve(0, rows)
        return rows

    def turn_resolve(self, pass_no: int, rows: Optional[torch.Tensor] = None, new_actions: Optional[torch.Tensor] = None,
                     reward_rows: Optional[torch.Tensor] = None, action_rows: Optional[torch.Tensor] = None) -> None:
        """``sgw_turn_resolve``: pass ``pass_no`` (1, 2, ...; 0 = render the pre-move windows) of a speculative policy turn over
        ``speculation_rows(rows)``.  ``new_actions``: the policy's int64 output -- for every row (``[A * E]``, agent-major) in pass 1, for
        the previous pass's dirty rows (``spec_dirty(pass_no - 1)`` order) afterwards; it is written into ``self.actions`` first.  Envs
        without a dirty agent are committed (grid, positions, ``self.rewards``, ``total_reward``; and ``reward_rows`` float32 /
        ``action_rows`` int64 ``[A, E]``, e.g. the rows of a replay ring).  ``spec_dirty(pass_no)`` then says which rows to think about again."""
        rows = self.speculation_rows(rows)
        st = self._spec_state
        A, E = self.spec.num_agents, self.num_envs
        pn, n_new = 0, 0
        if new_actions is not None:
            check_tensor("new_actions", new_actions, torch.int64, (A * E,) if pass_no == 1 else (None,), self.device)
            if new_actions.numel() > A * E:
                refuse("new_actions", new_actions, torch.int64, f"at most {A * E} elements", self.device)
            pn, n_new = new_actions.data_ptr(), int(new_actions.numel())
        if reward_rows is not None:
            check_tensor("reward_rows", reward_rows, torch.float32, A * E, self.device)
        if action_rows is not None:
            check_tensor("action_rows", action_rows, torch.int64, A * E, self.device)
        self._call(self._lib.sgw_turn_resolve, self._h, self.grid.data_ptr(), self.agent_pos.data_ptr(), self.actions.data_ptr(), rows.data_ptr(),
                   int(rows.shape[2]), self.rewards.data_ptr(), self.total_reward.data_ptr(), st.data_ptr(),
                   self._spec_list.data_ptr(), self._spec_ctr.data_ptr(), pn or None, n_new,
                   None if reward_rows is None else reward_rows.data_ptr(),
                   None if action_rows is None else action_rows.data_ptr(), int(pass_no), self._stream())

    def spec_count(self, pass_no: int) -> int:
        """How many rows pass ``pass_no`` rewrote (synchronises: the one read-back per pass)."""
        return int(self._spec_ctr[pass_no & 7].item())

    def spec_dirty(self, pass_no: int) -> torch.Tensor:
        """The rows pass ``pass_no`` rewrote, as int64 indices ``agent * E + env`` into the flattened ``[A * E, N]`` rows (synchronises: the
        host reads the count)."""
        n = int(self._spec_ctr[pass_no & 7].item())
        return self._spec_list[pass_no & 1, :n]

    def turn_prev_rows(self, agent: int, count: int, out: torch.Tensor) -> torch.Tensor:
        """``sgw_turn_prev_rows``: ``Buffer.current_state`` by the device's row count -- the ``count`` rows of the agent's bound replay
        states before the row the turn in flight fills, oldest first, into ``out`` ``[count, E, row_elems]`` (contiguous, the engine's
        observation dtype, on the device)."""
        bound = getattr(self, "_turn_row_elems", None) or ()
        row = bound[agent] if 0 <= agent < len(bound) else 0
        if not row:
            raise ValueError(f"agent {agent} has no replay states bound (turn_bind)")
        count, E = int(count), self.num_envs
        if check_tensor("out", out, self.obs_dtype, (count, E, ...), self.device).numel() != count * E * row:
            refuse("out", out, self.obs_dtype, f"[{count}, {E}] rows of {row} elements, the bound ring's row length,", self.device)
        self._call(self._lib.sgw_turn_prev_rows, self._h, int(agent), int(count), out.data_ptr(), self._stream())
        return out

    def turn_epsilon(self, epsilon: float, agent: int = -1):
        """``sgw_turn_epsilon``: the exploration rate of action-value acts (``turn_act*`` with float32 ``[E, n_actions]``) of one agent, or of
        every agent (``-1``): with that probability the act takes the engine's own uniform draw for (env, turn, agent) instead of the
        row's argmax.  Stream-ordered, kept on the device: a recorded turn follows it."""
        self._call(self._lib.sgw_turn_epsilon, self._h, int(agent), float(epsilon), self._stream())

    def turn_state(self):
        """(epoch, turn, [row per agent]) as the device has counted them (synchronising)."""
        et = (C.c_uint32 * 2)()
        rows = (C.c_int64 * N.MAX_AGENTS)()
        self._call(self._lib.sgw_turn_state, self._h, et, rows, self._stream())
        return int(et[0]), int(et[1]), [int(rows[a]) for a in range(self.spec.num_agents)]

    def observe_full(self, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The whole map as an observation, ``[E, C, H, W]`` (``ObservationSpec(full_view=True).observe``): every cell's
        appearance summed over the layers."""
        want = (self.num_envs, self.spec.num_channels, self.spec.height, self.spec.width)
        out = torch.empty(want, dtype=self.obs_dtype, device=self.device) if out is None else check_tensor("out", out, self.obs_dtype, want, self.device)
        self._call(self._lib.sgw_observe_full, self._h, self.grid.data_ptr(), out.data_ptr(), self._stream())
        return out

    def pick_obs_placement(self, candidates: int = 4, launches: int = 30) -> dict:
        """Where the observation tensor lies in device memory moves the launch time of kernels that write it with many small stores -- config
        5's walking workgroups: 83 ... 92 us for the same kernel on the same card, stable per allocation, indifferent to the offset inside one
        (``profiles/r05_c5_placement.txt``).  This allocates ``candidates`` observation tensors, times ``launches`` fused turns on each (the state
        tensors are restored afterwards) and keeps the fastest as ``self.obs``.  Returns the timings.  A no-op without an observation tensor."""
        if self.obs is None or candidates < 2:
            return {"candidates_us": [], "picked": 0}
        keep = {k: getattr(self, k).clone() for k in ("grid", "agent_pos", "actions", "rewards", "total_reward")}
        epoch, turn = self.epoch, self.turn
        tried, times = [self.obs], []
        for _ in range(candidates - 1):
            tried.append(torch.zeros_like(self.obs))
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for cand in tried:
            self.obs = cand
            for _ in range(launches):           # (warm: the first launches after an idle run slower)
                self.step(random_actions=True)
            ev0.record()
            for _ in range(launches):
                self.step(random_actions=True)
            ev1.record()
            torch.cuda.synchronize(self.device)
            times.append(ev0.elapsed_time(ev1) / launches * 1e3)
        best = min(range(len(tried)), key=lambda i: times[i])
        self.obs = tried[best]
        for k, v in keep.items():
            getattr(self, k).copy_(v)
        self.epoch, self.turn = epoch, turn
        self.status()                           # (whatever the timing turns flagged is theirs)
        del tried
        torch.cuda.empty_cache()
        return {"candidates_us": [round(t, 2) for t in times], "picked": best}

    def scratch_obs(self) -> torch.Tensor:
        if self._scratch_obs is None:
            self._scratch_obs = torch.zeros((self.num_envs,) + self.spec.obs_shape, dtype=self.obs_dtype, device=self.device)
        return self._scratch_obs

    def step(self, actions: Optional[torch.Tensor] = None, *, random_actions: bool = False, sweep: bool = True,
             write_obs: bool = True, agent_begin: int = 0, agent_end: Optional[int] = None,
             turn: Optional[int] = None, advance_turn: bool = True, obs_out: Optional[torch.Tensor] = None,
             obs_next: bool = False, obs_next_out: Optional[torch.Tensor] = None, no_move: bool = False, agent_major: bool = False):
        """One ``Environment.take_turn`` for every env (K2).

        ``actions``: uint8 ``[E, A]`` chosen by a policy; or ``random_actions=True``
        to draw them on device from the counter RNG (they are stored to
        ``self.actions``).  ``obs_next=True`` (policy-driven stepping): instead of the stepped
        agents' own observations, write the observation of agent ``agent_end`` as it stands
        after their moves -- into slot ``agent_end`` of the observation tensor, or, with
        ``obs_next_out`` (contiguous, the engine's observation dtype, ``E * C * V * V`` elements:
        e.g. a row of that agent's replay buffer), straight into that one-window-per-env tensor.
        ``no_move=True``: nobody acts -- the sweep (if ``sweep``) and the windows of the agents from the grid after it
        (steps 1 + 2 of a policy-driven turn in one launch; ``act`` then moves the agents one by one).
        With ``set_auto_reset`` armed, the call that completes turn
        ``max_turns`` also resets every env for the next epoch (``self.epoch`` / ``self.turn``
        follow when the engine keeps the counters, i.e. ``turn`` is not passed)."""
        if advance_turn and turn is None:
            self.turn += 1
        t = self.turn if turn is None else int(turn)
        if actions is not None and actions is not self.actions:
            # the step always consumes self.actions (so it also records what was taken)
            self.actions.copy_(actions.to(device=self.device, dtype=torch.uint8).reshape(self.actions.shape))
        actions = self.actions
        flags = (N.STEP_SWEEP if sweep else 0) | (N.STEP_RANDOM_ACTIONS if random_actions else 0) | (N.STEP_NO_MOVE if no_move else 0)
        if agent_major:      # obs_out is [A, E, C*V*V] (SGW_STEP_OBS_AGENT_MAJOR: engines with CAP_OBS_AGENT_MAJOR, whole-turn calls)
            obs = self.speculation_rows(obs_out)
            flags |= N.STEP_OBS_AGENT_MAJOR
        else:
            obs = self.obs if obs_out is None else self._check_obs(obs_out, "obs_out")
        if obs_next_out is not None:
            if not obs_next:
                raise ValueError("obs_next_out is the destination of obs_next=True")
            obs = self._check_window(obs_next_out, "obs_next_out")
            flags |= N.STEP_OBS_NEXT | N.STEP_OBS_NEXT_PACKED
        elif obs_next:
            if obs is None:
                raise ValueError("obs_next needs an observation tensor")
            flags |= N.STEP_OBS_NEXT
        elif not write_obs or obs is None:
            flags |= N.STEP_NO_OBS
            obs = None
        agent_end = self.spec.num_agents if agent_end is None else agent_end
        epoch = self.epoch
        self._call(self._lib.sgw_step, self._h, self.grid.data_ptr(), self.agent_pos.data_ptr(), actions.data_ptr(),
                   None if obs is None else obs.data_ptr(), self.rewards.data_ptr(), self.total_reward.data_ptr(),
                   epoch, t, agent_begin, agent_end, flags, self._stream())
        if self.max_turns and t == self.max_turns and agent_end == self.spec.num_agents and not no_move:
            self.epoch = epoch + 1        # the library has reset every env for the next epoch (sgw_set_auto_reset)
            if turn is None:
                self.turn = 0
        return obs, self.rewards

    def rollout(self, turns: int, *, random_actions: bool = True, actions: Optional[torch.Tensor] = None, sweep: bool = True,
                obs_out: Optional[torch.Tensor] = None, actions_out: Optional[torch.Tensor] = None,
                rewards_out: Optional[torch.Tensor] = None, write_obs: bool = True):
        """``turns`` whole ``take_turn``s with one call (``sgw_rollout``): where the kernel supports it they run inside one
        launch with every env's grid resident in LDS.  Without ``*_out`` tensors each turn overwrites ``self.obs`` /
        ``self.actions`` / ``self.rewards`` (they hold the last turn afterwards, as after ``turns`` calls of ``step``).
        ``obs_out [T, E, A, C, V, V]``, ``actions_out`` / ``rewards_out [T, E, A]`` (contiguous, the engine's dtypes)
        receive every turn -- e.g. ``T`` consecutive slots of a ``TurnBuffer``.  ``actions [T, E, A]``: scripted actions
        instead of on-device random ones."""
        T = int(turns)
        if T <= 0:
            return
        E, A = self.num_envs, self.spec.num_agents

        def per_turn(t, name, dtype, tail):
            """A caller-owned ``[T, *tail]`` tensor the kernels fill turn by turn through a raw pointer."""
            return check_tensor(name, t, dtype, (T,) + tuple(tail), self.device), math.prod(tail)

        flags = N.STEP_SWEEP if sweep else 0
        if actions is not None:                                  # scripted
            act, ts_act = per_turn(actions, "actions", torch.uint8, (E, A))
        elif not random_actions:
            raise ValueError("rollout needs random_actions=True or an actions tensor")
        else:
            flags |= N.STEP_RANDOM_ACTIONS
            act, ts_act = (self.actions, 0) if actions_out is None else per_turn(actions_out, "actions_out", torch.uint8, (E, A))
        rew, ts_rew = (self.rewards, 0) if rewards_out is None else per_turn(rewards_out, "rewards_out", torch.float32, (E, A))
        obs, ts_obs = (self.obs, 0) if obs_out is None else per_turn(obs_out, "obs_out", self.obs_dtype, (E,) + tuple(self.spec.obs_shape))
        if not write_obs or obs is None:
            flags |= N.STEP_NO_OBS
            obs = None
        self._call(self._lib.sgw_rollout, self._h, self.grid.data_ptr(), self.agent_pos.data_ptr(), act.data_ptr(),
                   None if obs is None else obs.data_ptr(), rew.data_ptr(), self.total_reward.data_ptr(), self.epoch, self.turn + 1, T,
                   ts_obs, ts_act, ts_rew, flags, self._stream())
        # the engine's own per-turn tensors hold the LAST turn, as after T calls of step()
        if act is not self.actions:
            self.actions.copy_(act[-1])
        if rew is not self.rewards:
            self.rewards.copy_(rew[-1])
        self.turn += T
        while self.max_turns and self.turn >= self.max_turns:    # the library reset the batch at every epoch boundary it crossed
            self.turn -= self.max_turns
            self.epoch += 1

    def set_auto_reset(self, max_turns: int):
        """Arm (``max_turns > 0``) or disarm the in-stream reset at the end of turn ``max_turns``;
        ``self.episode_return`` then holds each env's ``total_reward`` of the epoch that just ended."""
        self.max_turns = int(max_turns)
        if self.max_turns and self.episode_return is None:
            self.episode_return = torch.zeros((self.num_envs,), dtype=torch.float64, device=self.device)
        self._call(self._lib.sgw_set_auto_reset, self._h, self.max_turns, self.episode_return.data_ptr() if self.max_turns else None)

    def random_actions(self, turn: Optional[int] = None):
        t = self.turn + 1 if turn is None else int(turn)
        self._call(self._lib.sgw_random_actions, self._h, self.actions.data_ptr(), self.epoch, t, self._stream())
        return self.actions

    def reduce_metrics(self) -> torch.Tensor:
        """Device tensor ``[sum(total_reward), sum(total_reward**2), E, 0]`` (K4)."""
        self._call(self._lib.sgw_reduce_metrics, self._h, self.total_reward.data_ptr(), self.metrics.data_ptr(), self._stream())
        return self.metrics

    def status(self) -> int:
        """Synchronising read-and-clear of the device status word."""
        v = C.c_int32(0)
        self._call(self._lib.sgw_get_status, self._h, C.byref(v), self._stream())
        return int(v.value)

    def raise_on_status(self):
        s = self.status()
        if s & N.STATUS_OOB_MOVE:
            raise IndexError("an agent moved off the grid: the agent layer's border must be impassable "
                             "(the reference has no bounds check in Gridworld.move)")
        if s & N.STATUS_BAD_ACTION:
            raise KeyError("action index outside the ActionSpec")
        if s & N.STATUS_BAD_TYPE:
            raise KeyError("grid holds an entity type id that was never registered")
        if s & N.STATUS_BAD_POS:
            raise IndexError("an agent position outside the grid was passed to the engine")

    # ------------------------------------------------------------------ timing
    def set_timing(self, enable: bool):
        self._call(self._lib.sgw_set_timing, self._h, 1 if enable else 0)

    def step_time_ms(self):
        ms, n = C.c_double(0.0), C.c_int64(0)
        self._call(self._lib.sgw_get_step_time_ms, self._h, C.byref(ms), C.byref(n))
        return float(ms.value), int(n.value)

    def step_times_ms(self, capacity: int = 1 << 16):
        """Per-launch durations (ms, HIP events on the launch stream) since the last read, oldest first."""
        buf = (C.c_float * capacity)()
        n = C.c_int64(0)
        rc = self._lib.sgw_get_step_times_ms(self._h, buf, capacity, C.byref(n))      # (not through _call: 1 means "truncated", not an error)
        if rc < 0:
            N.check(rc)
        self.series_truncated = rc == 1          # launches beyond `capacity` / the library's sample cap were left out
        return [float(buf[i]) for i in range(int(n.value))]

    def set_wg_per_cu(self, n: int):
        """Launch tuning of the wave-per-env kernel: 0 automatic, 1..8 forced, -1 never capped (include/sgw.h)."""
        self._call(self._lib.sgw_set_wg_per_cu, self._h, int(n))

    def launch_info(self) -> str:
        buf = C.create_string_buffer(1024)
        self._call(self._lib.sgw_launch_info, self._h, buf, 1024)
        return buf.value.decode()
