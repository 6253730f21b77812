"""IQN's Q-network (``sorrel/models/pytorch/iqn.py:51-167`` and ``layers.py``'s ``NoisyLinear``): the modules, with the reference's
parameter and buffer names and shapes so that its ``state_dict`` loads, and the forward pass on the device.

* ``IQN.forward(input, n_tau)`` is the reference's sequence of torch ops: it supports autograd, runs on the CPU and is the baseline.  The
  ops are written once, in ``IQN.forward_flat``; every entry point that gets CPU tensors, the learner's CPU step included, calls it.
* ``IQN.quantiles`` / ``IQN.get_qvalues`` run ``sgw_iqn_forward`` (``sorrel_amd/csrc/iqn_forward.h``: two launches, nothing of size
  ``[B N, L]`` through memory) for device tensors, without autograd: acting, and the two ``next_states`` calls of a learner's step.  The
  taus are given, or drawn KEYED by (seed, env, epoch, turn, agent, quantile) so that a recorded turn draws fresh ones on every replay.
* ``IQN.forward_fused`` gives ``forward``'s results with autograd on the device: ``sgw_iqn_forward`` forwards, one ``sgw_iqn_backward``
  call (``sorrel_amd/csrc/iqn_backward.h``) backwards: the ``q_expected`` call of a learner's step.
* ``IQNActor`` is a ``BaseModel`` around an ``IQN`` whose ``take_action`` returns the float32 ``[E, A]`` action values: the act launch takes
  the argmax and explores (``SGW_ACT_QF32``).  It has no ``train_step``, no optimiser and no target network.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from sorrel_amd import _native as N_
from sorrel_amd.models.base_model import BaseModel

N_COS, MAX_LAYER, MAX_QUANTILES, MAX_ACTIONS = N_.IQN_N_COS, N_.IQN_MAX_LAYER, N_.IQN_MAX_QUANTILES, N_.IQN_MAX_ACTIONS    # (the header's)
# the ten weight fields of SgwIqnForwardDesc and SgwIqnBackwardDesc (the latter's gradients: "out_" + name), in the order of IQN.weight_list
WEIGHT_FIELDS = ("w_head", "b_head", "w_cos", "b_cos", "w_ff", "b_ff", "w_adv", "b_adv", "w_val", "b_val")


def fill_network_desc(d, flat=None, ws=None, sizes=None):
    """What ``SgwIqnForwardDesc`` and ``SgwIqnBackwardDesc`` share, over checked arguments: the states of a call (``flat`` ``[B, D]``), the
    ten weights (``ws``) and the network's ``sizes`` ``(L, N, A)``; a part that is None is left as it is."""
    if flat is not None:
        B, D = flat.shape
        d.states, d.n, d.in_features = flat.data_ptr(), B, D
        d.state_stride = int(flat.stride(0)) if B > 1 else max(int(flat.stride(0)), D)      # (one row: its stride is arbitrary)
        d.state_type = N_.IQN_STATE_U8 if flat.dtype == torch.uint8 else N_.IQN_STATE_F32
    if ws is not None:
        for name, w in zip(WEIGHT_FIELDS, ws):
            setattr(d, name, w.data_ptr())
    if sizes is not None:
        d.layer_size, d.num_quantiles, d.num_actions = sizes
        d.n_cos = N_COS


class NoisyLinear(nn.Linear):
    """``layers.py:9-65``: a linear layer whose training-mode weights are ``weight + sigma_weight * epsilon_weight`` with fresh normal
    ``epsilon`` per call; in eval mode the mean weights."""

    def __init__(self, in_features: int, out_features: int, sigma_init: float = 0.017, bias: bool = True) -> None:
        super().__init__(in_features, out_features, bias=bias)
        self.sigma_weight = nn.Parameter(torch.full((out_features, in_features), sigma_init))
        self.register_buffer("epsilon_weight", torch.zeros(out_features, in_features))
        if bias:
            self.sigma_bias = nn.Parameter(torch.full((out_features,), sigma_init))
            self.register_buffer("epsilon_bias", torch.zeros(out_features))
        self.reset_parameters()

    def reset_parameters(self) -> None:
        std = math.sqrt(3 / self.in_features)
        self.weight.data.uniform_(-std, std)
        self.bias.data.uniform_(-std, std)

    def effective(self, resample: bool = True, eps=None, noisy: Optional[bool] = None):
        """The (weight, bias) this layer applies now: in training mode (``noisy`` overrides it) ``weight + sigma * epsilon`` after new
        noise is drawn (``resample``, as ``forward`` does) or an ``eps`` pair (weight, bias) is copied into the epsilon buffers; else the
        mean weights."""
        if not (self.training if noisy is None else noisy):
            return self.weight, self.bias
        if eps is not None:
            self.epsilon_weight.copy_(eps[0])
        elif resample:
            self.epsilon_weight.normal_()
        weight = self.weight + self.sigma_weight * self.epsilon_weight
        bias = None
        if self.bias is not None:
            if eps is not None:
                self.epsilon_bias.copy_(eps[1])
            elif resample:
                self.epsilon_bias.normal_()
            bias = self.bias + self.sigma_bias * self.epsilon_bias
        return weight, bias

    def forward(self, input: torch.Tensor) -> torch.Tensor:
        weight, bias = self.effective()
        return F.linear(input, weight, bias)


class IQNOutput:
    """What ``IQN.quantiles`` gives back: ``quantiles`` float32 ``[B, N, A]``, ``taus`` ``[B, N, 1]``, ``qvalues`` ``[B, A]`` (the mean over
    the quantiles) and, if asked for, ``cos`` ``[B, N, 64]``, else None.  Passed back as ``out=`` its tensors are overwritten in place."""

    __slots__ = ("quantiles", "taus", "qvalues", "cos", "_workspace", "_weights")

    def __init__(self, B: int, N: int, A: int, L: int, device, cos: bool = False):
        self.quantiles = torch.empty((B, N, A), dtype=torch.float32, device=device)
        self.taus = torch.empty((B, N, 1), dtype=torch.float32, device=device)
        self.qvalues = torch.empty((B, A), dtype=torch.float32, device=device)
        self.cos = torch.empty((B, N, N_COS), dtype=torch.float32, device=device) if cos else None
        self._workspace = N_.workspace(4 * B * L, device)       # (float32 [B, L])
        self._weights = None                  # training mode: where the effective noisy weights are composed (fixed addresses)

    def __repr__(self):
        return f"IQNOutput(n={self.quantiles.shape[0]}, num_quantiles={self.quantiles.shape[1]}, num_actions={self.quantiles.shape[2]})"


class IQN(nn.Module):
    """The IQN Q-network (``iqn.py:51-167``)."""

    def __init__(self, input_size: Sequence[int], action_space: int, layer_size: int, seed: int, n_quantiles: int, n_frames: int = 5,
                 device="cpu") -> None:
        super().__init__()
        self.seed = torch.manual_seed(seed)
        self.key_seed = int(seed)
        self.input_shape = np.array(input_size)
        self.state_dim = len(self.input_shape)
        self.action_space = action_space
        self.n_quantiles = n_quantiles
        self.n_cos = N_COS
        self.layer_size = layer_size
        self.pis = torch.FloatTensor([np.pi * i for i in range(1, self.n_cos + 1)]).view(1, 1, self.n_cos).to(device)
        self.device = device
        self.head1 = nn.Linear(int(n_frames * self.input_shape.prod()), layer_size)
        self.cos_embedding = nn.Linear(self.n_cos, layer_size)
        self.ff_1 = NoisyLinear(layer_size, layer_size)
        self.cos_layer_out = layer_size
        self.advantage = NoisyLinear(layer_size, action_space)
        self.value = NoisyLinear(layer_size, 1)
        self._calls = 0                       # the turn of an unkeyed device call's draws: every call draws other taus
        self.to(device)

    # ------------------------------------------------------------------------------------------------ the torch-op path (the baseline)
    def calc_cos(self, batch_size: int, n_tau: int = 8, taus=None):
        if taus is None:
            taus = torch.rand(batch_size, n_tau).unsqueeze(-1).to(self.pis.device)
        else:
            taus = taus.reshape(batch_size, n_tau, 1)
        cos = torch.cos(taus * self.pis)
        assert cos.shape == (batch_size, n_tau, self.n_cos), "cos shape is incorrect"
        return cos, taus

    def forward_flat(self, flat: torch.Tensor, n_tau: int, taus=None, noise: Optional[bool] = None, eps=None):
        """The network's torch ops over flat states ``[B, D]`` (not cast): ``(quantiles [B, N, A], taus [B, N, 1])``.  The taus are as
        given, or drawn first.  The noisy layers follow ``training`` (``noise`` None), apply noise whatever it says (True: fresh, or the
        six ``eps`` tensors, ``ff_1``, ``advantage``, ``value``, weight before bias) or use the mean weights (False)."""
        batch_size = flat.shape[0]
        eps = [None] * 3 if eps is None else [eps[0:2], eps[2:4], eps[4:6]]
        x = torch.relu(self.head1(flat))
        cos, taus = self.calc_cos(batch_size, n_tau) if taus is None else self.calc_cos(batch_size, n_tau, taus)      # (drawn: the reference's call)
        cos = cos.view(batch_size * n_tau, self.n_cos)
        cos = torch.relu(self.cos_embedding(cos))
        cos_x = cos.view(batch_size, n_tau, self.cos_layer_out)
        x = (x.unsqueeze(1) * cos_x).view(batch_size * n_tau, self.cos_layer_out)
        x = torch.relu(F.linear(x, *self.ff_1.effective(eps=eps[0], noisy=noise)))
        advantage = F.linear(x, *self.advantage.effective(eps=eps[1], noisy=noise))
        value = F.linear(x, *self.value.effective(eps=eps[2], noisy=noise))
        out = value + advantage - advantage.mean(dim=1, keepdim=True)
        return out.view(batch_size, n_tau, self.action_space), taus

    def forward(self, input: torch.Tensor, n_tau: int = 8):
        return self.forward_flat(input.view(input.size()[0], -1), n_tau)

    def _apply(self, fn, *args, **kwargs):
        super()._apply(fn, *args, **kwargs)
        self.pis = fn(self.pis)
        return self

    # ------------------------------------------------------------------------------------------------ the device path
    def weight_list(self, noisy="mean", resample: bool = True):
        """The ten tensors in the order of ``WEIGHT_FIELDS``, as they are (not detached).  The noisy layers' six are the mean parameters
        (``"mean"``), what the layers apply now (``"effective"``: ``NoisyLinear.effective(resample)``) or six tensors of the caller's."""
        layers = (self.ff_1, self.advantage, self.value)
        if isinstance(noisy, str):
            noisy = [t for layer in layers for t in (layer.effective(resample) if noisy == "effective" else (layer.weight, layer.bias))]
        return [self.head1.weight, self.head1.bias, self.cos_embedding.weight, self.cos_embedding.bias, *noisy]

    def effective_weights(self, out: Optional[IQNOutput] = None, resample: bool = True):
        """The ten tensors ``sgw_iqn_forward`` takes, detached: in eval mode the parameters themselves; in training mode
        ``weight + sigma * epsilon`` of the three noisy layers with fresh noise (``resample``), composed into ``out``'s storage if given."""
        with torch.no_grad():
            ws = self.weight_list("effective", resample)
            if self.training and out is not None:
                if out._weights is None:
                    out._weights = [torch.empty_like(t) for t in ws[4:]]
                for dst, src in zip(out._weights, ws[4:]):
                    dst.copy_(src)
                ws[4:] = out._weights
            return [w.detach() for w in ws]

    def _check_states(self, states):
        if not torch.is_tensor(states):
            raise TypeError(f"states must be a tensor, not {type(states).__name__}")
        if states.dtype not in (torch.float32, torch.uint8):
            raise TypeError(f"states must be float32 or uint8, not {states.dtype}")
        if states.dim() < 1:
            raise ValueError("states must be [B, ...]")
        B = int(states.shape[0])
        flat = states.reshape(B, -1)
        D = self.head1.in_features
        if flat.shape[1] != D:
            raise ValueError(f"states hold {flat.shape[1]} elements per row; the head layer takes {D}")
        if flat.stride(1) != 1 and B > 0 and D > 1:
            raise ValueError("the elements of a state row must be contiguous")
        return B, flat

    def quantiles(self, states, n_tau: Optional[int] = None, *, taus=None, key=None, out: Optional[IQNOutput] = None, cos: bool = False,
                  engine=None, agent: Optional[int] = None):
        """The quantiles of ``states`` (float32 or uint8 ``[B, ...]``), without autograd: an ``IQNOutput``.  ``taus`` (float32 ``[B, N]`` or
        ``[B, N, 1]``) are used as given; otherwise they are drawn keyed: ``key`` is a dict of ``seed``, ``epoch``, ``turn``, ``num_envs``,
        ``agent0``, ``first_env`` and ``idx`` (all optional; without a key every call of this module draws other taus), or
        ``engine=, agent=`` runs ``sgw_turn_iqn_forward``, which reads epoch and turn from the engine's turn state (recordable).  Honours
        ``training``: the noisy layers' effective weights are composed first.  On a HIP device this is one ``sgw_iqn_forward`` call; with
        ``out=`` (an earlier result for the same shapes) it allocates nothing and does not synchronise.  CPU tensors run the torch ops."""
        B, flat, N, res = self._check_call(states, n_tau, taus, out, cos)
        dev = flat.device
        if dev.type != "cuda":
            with torch.no_grad():
                q, t = self.forward_flat(flat.float(), N, taus)
                res.quantiles.copy_(q)
                res.taus.copy_(t)
                res.qvalues.copy_(q.mean(dim=1))
                if res.cos is not None:
                    res.cos.copy_(self.calc_cos(B, N, t)[0])
            return res
        ws = self.effective_weights(res if out is not None else None)
        return self._launch_forward(flat, ws, res, taus, key, cos, engine, agent)

    def _check_call(self, states, n_tau, taus, out, cos: bool = False):
        """What ``quantiles`` and ``forward_fused`` ask of their arguments: ``(B, flat states, N, the IQNOutput to fill)``."""
        B, flat = self._check_states(states)
        N = int(self.n_quantiles if n_tau is None else n_tau)
        A, L = int(self.action_space), int(self.layer_size)
        if not 1 <= N <= MAX_QUANTILES:
            raise ValueError(f"{N} quantiles: the forward takes 1..{MAX_QUANTILES}")
        if not 1 <= A <= MAX_ACTIONS:
            raise ValueError(f"{A} actions: the forward takes 1..{MAX_ACTIONS}")
        if not 1 <= L <= MAX_LAYER:
            raise ValueError(f"layer_size = {L}: the forward takes 1..{MAX_LAYER}")
        dev = flat.device
        if self.head1.weight.device != dev:
            raise ValueError(f"states are on {dev}, the network on {self.head1.weight.device}")
        if taus is not None:
            if not torch.is_tensor(taus) or taus.dtype != torch.float32:
                raise TypeError("taus must be a float32 tensor")
            if tuple(taus.shape) not in ((B, N), (B, N, 1)) or not taus.is_contiguous() or taus.device != dev:
                raise ValueError(f"taus must be contiguous [{B}, {N}] or [{B}, {N}, 1] on {dev}; got {tuple(taus.shape)} on {taus.device}")
        if out is None:
            res = IQNOutput(B, N, A, L, dev, cos)
        else:
            if not isinstance(out, IQNOutput):
                raise TypeError("out= takes an earlier IQNOutput")
            if tuple(out.quantiles.shape) != (B, N, A) or out.quantiles.device != dev or out._workspace.numel() * 8 < 4 * B * L or (cos and out.cos is None):
                raise ValueError("out= was made for other shapes or another device, or without the optional outputs asked for")
            res = out
        return B, flat, N, res

    def _launch_forward(self, flat, ws, res: IQNOutput, taus=None, key=None, cos: bool = False, engine=None, agent: Optional[int] = None):
        """One ``sgw_iqn_forward`` call (or ``sgw_turn_iqn_forward``) over checked arguments: ``ws`` are the ten effective weights.
        ``key["clock"]`` (the device address of an ``sgw_learn_clock``) makes it ``sgw_iqn_forward_clocked``: the drawn taus' turn is the clock's."""
        B, N, A = res.quantiles.shape
        L, dev = int(self.layer_size), flat.device
        for w in ws:
            if w.dtype != torch.float32 or not w.is_contiguous():
                raise TypeError("the network's parameters must be contiguous float32")
        if B == 0:
            return res
        d = N_.SgwIqnForwardDesc()
        fill_network_desc(d, flat, ws, (L, N, A))
        d.out_qvalues, d.out_quantiles, d.out_taus = res.qvalues.data_ptr(), res.quantiles.data_ptr(), res.taus.data_ptr()
        if res.cos is not None and cos:
            d.out_cos = res.cos.data_ptr()
        d.workspace, d.workspace_bytes = res._workspace.data_ptr(), res._workspace.numel() * 8
        keep = clock = None
        if taus is not None:
            d.taus = taus.data_ptr()
        elif engine is None:
            key = dict(key or {})
            if not key:
                self._calls += 1
            d.seed = int(key.get("seed", self.key_seed)) & 0xFFFFFFFFFFFFFFFF
            d.epoch, d.turn = int(key.get("epoch", 0)), int(key.get("turn", self._calls)) & 0xFFFFFFFF
            d.num_envs, d.agent0, d.first_env = int(key.get("num_envs", max(B, 1))), int(key.get("agent0", 0)), int(key.get("first_env", 0))
            keep, clock = key.get("idx"), key.get("clock")
            if keep is not None:
                if keep.dtype != torch.int64 or tuple(keep.shape) != (B,) or not keep.is_contiguous() or keep.device != dev:
                    raise ValueError(f"key['idx'] must be contiguous int64 [{B}] on {dev}")
                d.idx = keep.data_ptr()
        if engine is not None and taus is None:
            if B != engine.num_envs:
                raise ValueError(f"the turn protocol's rows are the engine's {engine.num_envs} envs; got {B}")
            N_.launch("sgw_turn_iqn_forward", d, dev, engine._h, int(agent or 0))
        else:
            N_.launch("sgw_iqn_forward", d, dev, clock=clock)
        return res

    # ------------------------------------------------------------------------------------------------ the device path with autograd
    def forward_fused(self, states, n_tau: Optional[int] = None, *, taus=None, key=None, out: Optional[IQNOutput] = None):
        """``forward``'s results -- ``(quantiles [B, N, A], taus [B, N, 1])`` -- WITH autograd and without torch's network ops: on a HIP
        device the quantiles come from ``sgw_iqn_forward`` and their ``backward()`` is one ``sgw_iqn_backward`` call that hands the
        gradients of the ten effective weights to torch; those are composed with autograd (``weight + sigma * epsilon`` with fresh noise
        in training mode), so the gradients of ``weight`` and ``sigma_*`` follow by torch's own elementwise ops.  Nothing flows to the
        states or the taus.  ``taus`` and ``key`` as in ``quantiles``; ``out=`` (an ``IQNOutput``) is filled in place and must stay
        untouched until ``backward()`` has run: it holds the head layer's activations.  CPU tensors run ``forward``'s torch ops with the
        given taus."""
        B, flat, N, res = self._check_call(states, n_tau, taus, out)
        if flat.device.type != "cuda":
            return self.forward_flat(flat.float(), N, taus)
        quantiles = _FusedQuantiles.apply(self, flat, res, taus, key, *self.weight_list("effective"))
        return quantiles, res.taus

    def get_qvalues(self, inputs, n_tau: Optional[int] = None, **kwargs):
        """The mean of the quantiles, float32 ``[B, A]`` (``iqn.py:164-167``).  Tensors that require no kernel -- the CPU, or a call under
        autograd with ``requires_grad`` inputs -- take ``forward``; device tensors take ``quantiles`` (same keywords) and come detached."""
        if inputs.device.type != "cuda":
            if kwargs.get("taus") is None and kwargs.get("out") is None:
                quantiles, _ = self.forward(inputs, self.n_quantiles if n_tau is None else n_tau)
                return quantiles.mean(dim=1)
        return self.quantiles(inputs, n_tau, **kwargs).qvalues


class _FusedQuantiles(torch.autograd.Function):
    """``IQN.forward_fused`` on the device: ``sgw_iqn_forward`` forwards (``res`` keeps ``h`` and the taus), ``sgw_iqn_backward`` backwards."""

    @staticmethod
    def forward(ctx, net, flat, res, taus, key, *ws):
        ws = [w.detach().contiguous() for w in ws]
        net._launch_forward(flat, ws, res, taus, key)
        ctx.net_sizes = (int(net.layer_size), int(net.action_space))
        ctx.res = res                         # (h lives in its workspace, the taus in res.taus)
        ctx.shapes = [tuple(w.shape) for w in ws]
        ctx.save_for_backward(flat, *ws)
        return res.quantiles.view_as(res.quantiles)

    @staticmethod
    def backward(ctx, grad):
        flat, *ws = ctx.saved_tensors
        res = ctx.res
        L, A = ctx.net_sizes
        B, N = int(res.quantiles.shape[0]), int(res.quantiles.shape[1])
        dev = flat.device
        need = ctx.needs_input_grad[5:]
        grads = [torch.zeros(shape, dtype=torch.float32, device=dev) if wanted else None for shape, wanted in zip(ctx.shapes, need)]
        if B > 0 and any(need):
            grad = grad.to(torch.float32).contiguous()
            D = int(flat.shape[1])
            space = N_.workspace(int(N_.load().sgw_iqn_backward_workspace_bytes(B, D, L, N, A)), dev)
            d = N_.SgwIqnBackwardDesc()
            fill_network_desc(d, flat, ws, (L, N, A))
            d.taus, d.h, d.grad_quantiles = res.taus.data_ptr(), res._workspace.data_ptr(), grad.data_ptr()
            for name, g in zip(WEIGHT_FIELDS, grads):
                if g is not None:
                    setattr(d, "out_" + name, g.data_ptr())
            d.workspace, d.workspace_bytes = space.data_ptr(), space.numel() * 8
            N_.launch("sgw_iqn_backward", d, dev)
        return (None, None, None, None, None, *grads)


class IQNActor(BaseModel):
    """A policy that acts through an ``IQN``: ``take_action(state)`` returns the float32 ``[E, A]`` action values, so the act launch takes the
    argmax and explores with ``epsilon`` (``SGW_ACT_QF32``).  ``bind(env, slot)`` tells it whose turn its taus are keyed by: eagerly the
    environment's (seed, epoch, turn) go into the call; under ``capture_turn()`` it uses ``sgw_turn_iqn_forward``, which reads them on the
    device, so a replayed turn draws new taus.  No ``train_step``, no optimiser, no target network."""

    def __init__(self, input_size, action_space: int, layer_size: int = 250, n_quantiles: int = 12, n_frames: int = 1, seed: int = 0,
                 memory_size: int = 0, epsilon: float = 0.0, num_envs: int = 1, device=None):
        super().__init__(input_size, action_space, memory_size=memory_size, epsilon=epsilon, num_envs=num_envs, device=device)
        shape = tuple(input_size) if isinstance(input_size, Sequence) else (input_size,)
        self.net = IQN(shape, action_space, layer_size, seed, n_quantiles, n_frames=n_frames, device=device or "cpu")
        self.net.eval()
        self._env = None
        self._slot = 0
        self._out = None

    def bind(self, env, slot: int) -> "IQNActor":
        self._env, self._slot = env, int(slot)
        return self

    def take_action(self, state):
        q, self._out = act_values(self.net, state, self._out, self._env, self._slot, mean=False)
        return q


def act_values(net: IQN, state, out: Optional[IQNOutput], env, slot: int, mean: bool):
    """The float32 ``[E, A]`` action values of ``state`` without autograd, and the ``IQNOutput`` they live in (``out`` if it fits, else a new
    one; None on the CPU): what a bound model's ``take_action`` returns and keeps.  ``mean`` takes the mean weights whatever ``training``
    says; otherwise the network acts as ``quantiles`` does.  The taus are keyed by ``env``'s turn for agent ``slot`` (None: by the network's
    own count of calls): eagerly the environment's (seed, epoch, turn) go into the call, under ``capture_turn()`` the device reads them."""
    B = int(state.shape[0])
    if state.device.type != "cuda":
        with torch.no_grad():
            q, _ = net.forward_flat(state.reshape(B, -1).float(), net.n_quantiles, noise=False if mean else None)
            return q.mean(dim=1), None
    if out is None or out.quantiles.shape[0] != B or out.quantiles.device != state.device:
        out = IQNOutput(B, net.n_quantiles, net.action_space, net.layer_size, state.device)
    _, flat, _, res = net._check_call(state, None, None, out)
    ws = net.weight_list() if mean else net.effective_weights(res)
    key = eng = None
    if env is not None:
        eng = env._ensure_engine()
        if getattr(env, "_mixed", False):
            eng = env._agent_engine[slot]
        if not env._turn_capture:
            key = {"seed": int(eng.spec.seed), "epoch": int(env.epoch), "turn": int(env.turn), "num_envs": int(eng.num_envs), "agent0": slot,
                   "first_env": int(eng.first_env_id)}
            eng = None
    return net._launch_forward(flat, ws, res, key=key, engine=eng, agent=slot).qvalues, res
