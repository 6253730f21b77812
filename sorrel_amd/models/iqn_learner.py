"""The IQN learner (``sorrel/models/pytorch/iqn.py:179-443``: ``iRainbowModel``, which the reference's examples import as ``PyTorchIQN``): two
``IQN`` networks, Adam, a replay ``Buffer``, ``take_action``, ``train_step``, ``start_epoch_action``, ``save`` / ``load``.

* On the CPU ``train_step`` runs the reference's lines as torch ops: the baseline, and what the reference returns (a 0-d float32 ndarray).
* On a HIP device ``train_step`` is a fixed sequence of native calls over buffers allocated once, without autograd:
  ``sgw_sample`` (``ReplaySampler``), one ``sgw_noisy_weights`` call that composes the effective noisy weights of the three network calls
  (18 tensors; ``sorrel_amd/csrc/noisy.h``), three ``sgw_iqn_forward`` calls, ``sgw_iqn_loss``, one ``sgw_iqn_backward`` that writes into the
  parameters' persistent ``.grad`` tensors (the gradient of a noisy layer's ``weight`` IS that of its effective weight), one
  ``sgw_noisy_weights`` call in backward mode for the six ``sigma_*.grad``, and ``FusedAdam.step()`` (clipping, Adam and the soft update).
  The taus and the noise are keyed by (``seed``, the count of steps done, the network call's index 0..2): a step is reproducible from
  its number.  The loss comes back as a 0-d float32 device tensor, a view of a buffer the next call overwrites; nothing synchronises.
* ``capture_train_step()`` records that sequence once as a graph: the three scalars that change from step to step (the count, twice, and the
  ring's filled rows) then come from an ``sgw_learn_clock`` in device memory through the ``*_clocked`` twins of the three calls that take
  them, ``sgw_learn_clock_advance`` ends the chain, and ``train_step()`` is one replay.  ``updates_per_call`` makes several updates per call.
* ``take_action`` evaluates ``qnetwork_local`` with the MEAN weights (the reference acts in eval mode) and returns the float32 ``[E, A]``
  action values: the act launch takes the argmax and explores with ``epsilon``.  It never toggles ``training``."""
from __future__ import annotations

import os
from typing import Optional, Sequence

import numpy as np
import torch

from sorrel_amd import _native as N_
from sorrel_amd.buffers import Buffer, ReplaySampler
from sorrel_amd.models.base_model import BaseModel
from sorrel_amd.models.iqn import IQN, WEIGHT_FIELDS, IQNOutput, act_values, fill_network_desc
from sorrel_amd.optim import FusedAdam
from sorrel_amd.spec import resolve_device

NOISY_LAYERS = ("ff_1", "advantage", "value")
N_NOISE = 2 * len(NOISY_LAYERS)               # eps tensors of one network call: (weight, bias) of each noisy layer, in that order
N_CALLS = 3                                   # local on next_states, target on next_states, local on states


def _noisy_tensors(net: IQN):
    """``(weight-like, its sigma)`` of the six noisy tensors of ``net``, in the order the noise is drawn."""
    out = []
    for name in NOISY_LAYERS:
        layer = getattr(net, name)
        out += [(layer.weight, layer.sigma_weight), (layer.bias, layer.sigma_bias)]
    return out


class _DeviceStep:
    """What the device path of ``train_step`` allocates once: the three sets of effective weights, the kept noise, the three forwards'
    outputs, the loss terms, the backward's workspace and the descriptors whose pointers do not change."""

    __slots__ = ("key", "eff", "eps", "outs", "loss", "space", "noise_fwd", "noise_bwd", "bwd")


class _RecordedStep:
    """``capture_train_step``'s result: the graph and what it holds by address (compared on the host before every replay)."""

    __slots__ = ("graph", "prepare_key", "adam_key", "adam_tables", "sampler", "ring", "storage", "replays")


def _ring_storage(ring):
    return tuple(t.data_ptr() for t in (ring.states, ring.actions, ring.rewards, ring.dones))


class iRainbowModel(BaseModel):
    """The reference's ``iRainbowModel`` (its constructor, argument names and defaults), plus ``num_envs`` for the batched replay ring."""

    def __init__(self, input_size: Sequence[int], action_space: int, layer_size: int, epsilon: float, device, seed: int, n_frames: int,
                 n_step: int = 3, sync_freq: int = 200, model_update_freq: int = 4, batch_size: int = 64, memory_size: int = 1024,
                 LR: float = 0.001, TAU: float = 0.001, GAMMA: float = 0.99, n_quantiles: int = 12, num_envs: int = 1) -> None:
        super().__init__(input_size, action_space, memory_size=0, epsilon=epsilon)
        self.layer_size = layer_size
        self.device = resolve_device(device)
        self.key_seed = int(seed)
        self.seed = torch.manual_seed(seed)
        self.n_frames, self.TAU, self.n_quantiles, self.GAMMA = n_frames, TAU, n_quantiles, GAMMA
        self.batch_size, self.n_step, self.sync_freq, self.model_update_freq = batch_size, n_step, sync_freq, model_update_freq
        shape = tuple(input_size) if isinstance(input_size, Sequence) else (input_size,)
        self.qnetwork_local = IQN(shape, action_space, layer_size, seed, n_quantiles, n_frames, device=self.device)
        self.qnetwork_target = IQN(shape, action_space, layer_size, seed, n_quantiles, n_frames, device=self.device)
        self.models = {"local": self.qnetwork_local, "target": self.qnetwork_target}
        self.optimizer = FusedAdam(self.qnetwork_local.parameters(), lr=LR, max_grad_norm=1, target_params=self.qnetwork_target.parameters(), tau=TAU)
        self.memory = Buffer(capacity=memory_size, obs_shape=(int(np.array(shape).prod()),), n_frames=n_frames, num_envs=num_envs, device=self.device)
        self.steps_done = 0                   # the count of gated steps: the key of a step's taus and noise
        self._env, self._slot, self._out = None, 0, None
        self._sampler: Optional[ReplaySampler] = None
        self._step: Optional[_DeviceStep] = None
        self._loss32 = torch.zeros((), dtype=torch.float32, device=self.device)
        self.updates_per_call = 1             # gated steps of one train_step() without overrides (the reference makes one)
        self.capture_lazily = False           # record the step at the first gated train_step() (examples: config.model.capture_train_step)
        self.capture_error: Optional[BaseException] = None        # why a lazy capture was given up
        self._recorded: Optional[_RecordedStep] = None
        self._clock = None                    # the sgw_learn_clock's four words on the device, once a step was recorded
        self._clock_count = self._clock_starts = None             # ... as the host last wrote them (None: not known)

    def __str__(self):
        return f"iRainbowModel(input_size={np.array(self.input_size).prod() * self.n_frames},action_space={self.action_space})"

    # ------------------------------------------------------------------------------------------------------------ acting
    def bind(self, env, slot: int) -> "iRainbowModel":
        """Whose turn the taus of ``take_action`` are keyed by (as ``IQNActor.bind``)."""
        self._env, self._slot = env, int(slot)
        return self

    def take_action(self, state):
        """The float32 ``[E, A]`` action values of ``qnetwork_local`` with the mean weights, detached."""
        q, self._out = act_values(self.qnetwork_local, state, self._out, self._env, self._slot, mean=True)
        return q

    # ------------------------------------------------------------------------------------------------------------ the epoch hooks
    def start_epoch_action(self, **kwargs) -> None:
        self.memory.add_empty()
        if kwargs["epoch"] % self.sync_freq == 0:
            self.qnetwork_target.load_state_dict(self.qnetwork_local.state_dict())

    def end_epoch_action(self, **kwargs) -> None:
        pass

    def soft_update(self) -> None:
        """``target = TAU * local + (1 - TAU) * target`` (what ``train_step`` does inside the optimiser's call)."""
        for target_param, local_param in zip(self.qnetwork_target.parameters(), self.qnetwork_local.parameters()):
            target_param.data.copy_(self.TAU * local_param.data + (1.0 - self.TAU) * target_param.data)

    # ------------------------------------------------------------------------------------------------------------ files
    def save(self, file_path) -> None:
        """The reference's checkpoint: ``{"local": state_dict, "target": state_dict, "optim": the optimiser's}`` through ``torch.save``."""
        directory = os.path.dirname(str(file_path))
        if directory:
            os.makedirs(directory, exist_ok=True)
        torch.save({**{key: value.state_dict() for key, value in self.models.items()}, "optim": self.optimizer.state_dict()}, file_path)

    def load(self, file_path) -> None:
        checkpoint = torch.load(file_path, map_location=self.device)
        for key in self.models:
            self.models[key].load_state_dict(checkpoint[key])
        self.optimizer.load_state_dict(checkpoint["optim"])

    # ------------------------------------------------------------------------------------------------------------ the step
    def train_step(self, *, batch=None, taus=None, noise=None):
        """One update (``iqn.py:322-412``), gated by ``len(memory) > batch_size``.  Keyword-only test hooks override the draws on both
        paths: ``batch`` = the six-tuple ``Buffer.sample`` returns, ``taus`` = three ``[B, N]`` tensors and ``noise`` = 18 eps tensors, both in
        the order of the network calls (local on next_states, target on next_states, local on states; within a call ``ff_1``,
        ``advantage``, ``value``, weight before bias).  Returns the loss: on the CPU a 0-d float32 ndarray, on a HIP device a 0-d float32
        tensor that the next call overwrites (0 below the gate)."""
        if taus is not None and len(taus) != N_CALLS:
            raise ValueError(f"taus= takes {N_CALLS} tensors, one per network call")
        if noise is not None and len(noise) != N_CALLS * N_NOISE:
            raise ValueError(f"noise= takes {N_CALLS * N_NOISE} tensors, six per network call")
        overrides = batch is not None or taus is not None or noise is not None
        updates = 1 if overrides else max(1, int(self.updates_per_call))
        if self.device.type != "cuda":
            for _ in range(updates):
                loss = self._train_step_torch(batch, taus, noise)
            return loss
        if not len(self.memory) > self.batch_size:
            self._loss32.zero_()
            return self._loss32
        if overrides:
            self._train_step_device(batch, taus, noise)
            if self._recorded is not None:
                self._sync_clock()            # an eager step between replays leaves the clock at steps_done
            return self._loss32
        if self._recorded is None and self.capture_lazily:
            warmup = min(2, updates)          # the warm-up steps are real ones: they are this call's first updates
            try:
                self.capture_train_step(warmup=warmup)
                updates -= warmup
            except Exception as exc:          # not recordable here: say why once and stay eager
                self.capture_lazily, self.capture_error = False, exc
        for _ in range(updates):
            rec = self._recorded
            if rec is not None and not self._recording_holds(rec):
                self.release_train_step()     # something the graph holds by address has moved: eager, as without a recording
                rec = None
            if rec is None:
                self._train_step_device(None, None, None)
            else:
                self._sync_clock()
                rec.graph.replay()
                rec.replays += 1
                self.steps_done += 1
                self._clock_count += 1        # (sgw_learn_clock_advance ran on the device)
        return self._loss32

    def _train_step_torch(self, batch, taus, noise):
        from sorrel_amd.losses import _iqn_loss_torch         # (losses imports this package's base_model: not at module level)

        loss = torch.tensor(0.0)
        self.optimizer.zero_grad(set_to_none=True)        # (torch's default, which the reference's optimizer.zero_grad() takes)
        if len(self.memory) > self.batch_size:
            if batch is None:
                batch = self.memory.sample(batch_size=self.batch_size)
            states, actions, rewards, next_states, dones, valid = (torch.as_tensor(x) for x in batch)
            local, target, n = self.qnetwork_local, self.qnetwork_target, self.n_quantiles
            tau = [None] * N_CALLS if taus is None else list(taus)
            eps = [None] * N_CALLS if noise is None else [noise[c * N_NOISE:(c + 1) * N_NOISE] for c in range(N_CALLS)]
            B = states.shape[0]
            q_next_local, _ = local.forward_flat(next_states.view(B, -1), n, tau[0], noise=True, eps=eps[0])
            q_next_target, _ = target.forward_flat(next_states.view(B, -1), n, tau[1], noise=True, eps=eps[1])
            q_expected, t = local.forward_flat(states.view(B, -1), n, tau[2], noise=True, eps=eps[2])
            loss = _iqn_loss_torch(q_expected, t, q_next_local, q_next_target, actions, rewards, dones, valid, self.GAMMA ** self.n_step)[0]
            loss.backward()
            self.optimizer.step()             # clip_grad_norm_(.., 1), Adam, soft_update(): the reference's lines (optim._adam_step_torch)
            self.steps_done += 1
        return loss.detach().numpy()

    def _prepare_key(self):
        """Where the parameters, their gradients and the target's parameters lie (None while a gradient is missing)."""
        params = list(self.qnetwork_local.parameters())
        if any(p.grad is None for p in params):
            return None
        return (tuple(p.data_ptr() for p in params) + tuple(p.grad.data_ptr() for p in params)
                + tuple(p.data_ptr() for p in self.qnetwork_target.parameters()))

    def _prepare(self) -> _DeviceStep:
        """The device step's buffers and descriptors, rebuilt only when a parameter or a gradient has moved."""
        from sorrel_amd.losses import IQNLoss

        local, target = self.qnetwork_local, self.qnetwork_target
        params = list(local.parameters())
        for p in params:
            if p.grad is None:
                p.grad = torch.zeros_like(p)
        key = self._prepare_key()
        st = self._step
        if st is not None and st.key == key:
            return st
        dev, B, Nq, A, L = self.device, self.batch_size, self.n_quantiles, self.action_space, self.layer_size
        D = local.head1.in_features
        if st is None:
            st = _DeviceStep()
            st.eff = [[torch.empty_like(w) for w, _ in _noisy_tensors(local)] for _ in range(N_CALLS)]
            st.eps = [torch.empty_like(w) for w, _ in _noisy_tensors(local)]
            st.outs = [IQNOutput(B, Nq, A, L, dev) for _ in range(N_CALLS)]
            st.loss = IQNLoss(st.outs[2].quantiles)
            st.space = N_.workspace(int(N_.load().sgw_iqn_backward_workspace_bytes(B, D, L, Nq, A)), dev)
        st.key = key
        # the forward composition: job c * 6 + t = tensor t of network call c (the target network in call 1)
        f = N_.SgwNoisyWeightsDesc()
        f.mode, f.num_jobs, f.seed = N_.NOISY_FORWARD, N_CALLS * N_NOISE, self.key_seed & 0xFFFFFFFFFFFFFFFF
        for c, net in enumerate((local, target, local)):
            for t, (w, s) in enumerate(_noisy_tensors(net)):
                job = f.jobs[c * N_NOISE + t]
                job.weight, job.sigma, job.out_eff, job.count, job.tensor_id = w.data_ptr(), s.data_ptr(), st.eff[c][t].data_ptr(), w.numel(), c * N_NOISE + t
                if c == N_CALLS - 1:
                    job.out_eps = st.eps[t].data_ptr()        # the backward needs the noise of the q_expected call, drawn or given
        st.noise_fwd = f
        g = N_.SgwNoisyWeightsDesc()
        g.mode, g.num_jobs = N_.NOISY_BACKWARD, N_NOISE
        for t, (w, s) in enumerate(_noisy_tensors(local)):
            job = g.jobs[t]
            job.grad_eff, job.eps_in, job.out_grad_sigma, job.count = w.grad.data_ptr(), st.eps[t].data_ptr(), s.grad.data_ptr(), w.numel()
        st.noise_bwd = g
        d = N_.SgwIqnBackwardDesc()               # (the states of a step go in when it runs)
        fill_network_desc(d, ws=local.weight_list(st.eff[2]), sizes=(L, Nq, A))
        res = st.outs[2]
        d.taus, d.h, d.grad_quantiles = res.taus.data_ptr(), res._workspace.data_ptr(), st.loss.grad_expected.data_ptr()
        for name, w in zip(WEIGHT_FIELDS, local.weight_list()):
            setattr(d, "out_" + name, w.grad.data_ptr())
        d.workspace, d.workspace_bytes = st.space.data_ptr(), st.space.numel() * 8
        st.bwd = d
        self._step = st
        return st

    def _train_step_device(self, batch, taus, noise, clock=None):
        """The step's launches.  ``clock`` (the device address of the learner clock; no overrides then): the clocked twins of the three calls
        that take the step's count or the ring's filled rows, and ``sgw_learn_clock_advance`` behind the optimiser -- what a graph records."""
        from sorrel_amd.losses import iqn_loss_terms

        dev, B = self.device, self.batch_size
        local, target = self.qnetwork_local, self.qnetwork_target
        if batch is None:
            batch = self._ensure_sampler().sample(clock=clock)
        states, actions, rewards, next_states, dones, valid = batch
        if int(states.shape[0]) != B or int(next_states.shape[0]) != B:
            raise ValueError(f"batch= holds {int(states.shape[0])} states; the learner's batch_size is {B}")
        st = self._prepare()
        step = self.steps_done if clock is None else 0          # (clocked: the kernels read the count on the device)
        # 1: the effective noisy weights of the three network calls
        f = st.noise_fwd
        f.draw = step & 0xFFFFFFFFFFFFFFFF
        for k in range(N_CALLS * N_NOISE):
            eps = None if noise is None else noise[k]
            if eps is not None and (eps.dtype != torch.float32 or eps.device != dev or not eps.is_contiguous() or eps.numel() != f.jobs[k].count):
                raise ValueError(f"noise[{k}] must be a contiguous float32 tensor of {f.jobs[k].count} elements on {dev}")
            f.jobs[k].eps_in = None if eps is None else eps.data_ptr()
        N_.launch("sgw_noisy_weights", f, dev, clock=clock)
        # 2: the three forwards; the third keeps h (its workspace) and its taus
        for c, (net, x) in enumerate(((local, next_states), (target, next_states), (local, states))):
            _, flat, _, res = net._check_call(x, self.n_quantiles, None if taus is None else taus[c], st.outs[c])
            key = {"seed": self.key_seed, "epoch": c, "turn": step & 0xFFFFFFFF, "num_envs": B, "clock": clock}
            net._launch_forward(flat, net.weight_list(st.eff[c]), res, None if taus is None else taus[c], key)
        # 3: the loss and its gradient at q_expected
        q = st.outs
        iqn_loss_terms(q[2].quantiles, q[2].taus, q[0].quantiles, q[1].quantiles, actions, rewards, dones, valid, self.GAMMA ** self.n_step, out=st.loss)
        # 4: the backward into the parameters' gradients, then the sigmas'
        fill_network_desc(st.bwd, states.reshape(B, -1))
        N_.launch("sgw_iqn_backward", st.bwd, dev)
        N_.launch("sgw_noisy_weights", st.noise_bwd, dev)
        # 5: clipping, Adam and the soft update
        self.optimizer.step()
        self.steps_done += 1
        self._loss32.copy_(st.loss.loss)
        if clock is not None:
            index = dev.index if dev.index is not None else torch.cuda.current_device()
            N_.call(index, N_.load().sgw_learn_clock_advance, clock, N_.raw_stream(index))      # the chain's last node: the next step's key
        return self._loss32

    def _ensure_sampler(self) -> ReplaySampler:
        if self._sampler is None or self._sampler.ring is not self.memory:
            self._sampler = ReplaySampler(self.memory, self.batch_size, seed=self.key_seed)
        return self._sampler

    # ------------------------------------------------------------------------------------------------------------ the recorded step
    def _sync_clock(self) -> None:
        """The host's view into the clock, stream-ordered, where it differs from what was last written: nothing is launched while replays follow
        each other on a full ring."""
        starts = self._ensure_sampler().num_starts()
        if self._clock_count != self.steps_done:
            self._clock[0].fill_(self.steps_done)
            self._clock_count = self.steps_done
        if self._clock_starts != starts:
            self._clock[1].fill_(starts)
            self._clock_starts = starts

    def _recording_holds(self, rec: _RecordedStep) -> bool:
        """Does everything the graph holds by address still lie where it was recorded?  (Host arithmetic only.)"""
        opt, st = self.optimizer, self._step
        return (st is not None and st.key == rec.prepare_key and self._prepare_key() == rec.prepare_key
                and opt._key is rec.adam_key and opt._tables is rec.adam_tables and opt.table_key() == rec.adam_key
                and self._sampler is rec.sampler and rec.sampler.ring is self.memory and self.memory is rec.ring
                and _ring_storage(self.memory) == rec.storage)

    def _host_counters(self):
        return (self.steps_done, self.memory.idx, self.memory.size, [(tb, tb.step, tb.pending) for tb in self.optimizer._tables])

    def _restore_host_counters(self, saved) -> None:
        self.steps_done, self.memory.idx, self.memory.size = saved[:3]
        for tb, step, pending in saved[3]:
            tb.step, tb.pending = step, pending

    def capture_train_step(self, warmup: int = 2) -> _RecordedStep:
        """Record the device path of ``train_step`` -- ``_train_step_device`` itself, with the clocked twins of the three calls that take the
        step's count or the ring's filled rows -- as ONE graph, and return the recorded object.  Afterwards ``train_step()`` without overrides
        checks on the host that nothing the graph holds by address has moved, writes the ring's ``num_starts`` into the clock when it changed,
        replays and counts; when something has moved (``load``, ``optimizer.load_state_dict``, a new ring) the recording is dropped and the
        call runs eagerly, as does every call with overrides.  ``release_train_step()`` drops it on request.

        ``warmup`` (at least 1) REAL steps run first, on a side stream, through the same clocked calls: they count, and they build everything
        that uploads or allocates (descriptors, the sampler, Adam's table) before the capture begins.  The optimiser is switched to
        ``device_step=True`` (``FusedAdam.count_on_device``), whose bias corrections are running products of the betas: a recorded step equals,
        bit for bit, the eager step of a model whose optimiser ALSO counts on the device -- not the default one's, which uses ``pow``.
        Raises ``RuntimeError`` on a CPU model or below the gate; when the capture itself fails, the host's counters are put back, the
        optimiser's counting is as it was, and the model is in its eager state."""
        if self.device.type != "cuda":
            raise RuntimeError("capture_train_step: the model is on the CPU, where train_step is torch ops with autograd; only the device path "
                               "is a fixed sequence of launches")
        if not len(self.memory) > self.batch_size:
            raise RuntimeError(f"capture_train_step: the gate is closed (len(memory) = {len(self.memory)} <= batch_size = {self.batch_size}): "
                               "there is no step to record yet")
        self.release_train_step()
        counted_on_device = self.optimizer.device_step
        try:
            rec = self._record(max(1, int(warmup)))
        except BaseException:
            self._recorded = None
            self._clock_count = self._clock_starts = None
            self.optimizer.count_on_device(counted_on_device)
            raise
        self._recorded = rec
        return rec

    def _warm_up(self, steps: int, clock: int) -> None:
        """``steps`` real steps through the clocked calls on a side stream (as ``turns/recorded.py`` warms a turn up): they count, and they
        build the descriptors, the sampler and Adam's table, which upload or allocate."""
        dev = self.device
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(steps):
                self._sync_clock()
                self._train_step_device(None, None, None, clock=clock)
                self._clock_count += 1
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)

    def _record(self, warmup: int) -> _RecordedStep:
        from sorrel_amd import capture

        self.optimizer.count_on_device(True)
        if self._clock is None:
            self._clock = torch.zeros((4,), dtype=torch.int64, device=self.device)        # one allocation: 8-byte aligned
        self._clock_count = self._clock_starts = None
        clock = self._clock.data_ptr()
        self._warm_up(warmup, clock)
        rec = _RecordedStep()
        rec.graph, rec.replays = torch.cuda.CUDAGraph(), 0
        self._sync_clock()
        saved = self._host_counters()
        try:
            with capture.recording(rec.graph):
                self._train_step_device(None, None, None, clock=clock)       # recorded, not run: one stream, one chain
        finally:
            self._restore_host_counters(saved)                               # (also when the capture fails half-way)
        rec.prepare_key, rec.adam_key, rec.adam_tables = self._step.key, self.optimizer._key, self.optimizer._tables
        rec.sampler, rec.ring, rec.storage = self._sampler, self.memory, _ring_storage(self.memory)
        if [(tb, tb.step, tb.pending) for tb in rec.adam_tables] != saved[3] or not self._recording_holds(rec):
            raise RuntimeError("capture_train_step: a descriptor, the sampler or Adam's table was rebuilt inside the capture")
        return rec

    def release_train_step(self) -> None:
        """Drop the recording: ``train_step`` is the eager sequence again (the optimiser keeps counting on the device)."""
        self._recorded = None
