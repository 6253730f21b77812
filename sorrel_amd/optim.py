"""The learners' optimiser tail on the device.

What the reference runs after ``loss.backward()`` -- ``clip_grad_norm_(local.parameters(), 1)``, ``optimizer.step()`` and
``soft_update()`` in ``iRainbowModel.train_step`` (``sorrel/models/pytorch/iqn.py:405-410``), ``optimizer.step()`` over two parameter
groups in ``PyTorchPPO.train_step`` (``ppo.py:283-285``) -- is one ``sgw_adam_step`` call (``sorrel_amd/csrc/adam_step.h``) per dtype:
two launches for the whole parameter list, one when nothing is clipped.  A user's learner writes::

    optimizer = FusedAdam(local.parameters(), lr=LR, max_grad_norm=1, target_params=target.parameters(), tau=TAU)
    loss = iqn_loss(...); optimizer.zero_grad(); loss.backward(); optimizer.step()

``_adam_step_torch`` is the reference's lines as torch ops: the path of CPU tensors, and what the kernel is compared with and timed
against.  Device tensors always use the kernel.  The networks and the learner class stay the user's."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

_DTYPES = (torch.float32, torch.float64)


def _adam_step_torch(params, optimizer, max_grad_norm=None, target_params=None, tau=None):
    """The reference's lines: ``clip_grad_norm_``, the optimiser's step, the ``soft_update`` loop.  Returns the norm or None."""
    params = list(params)
    norm = None
    if max_grad_norm is not None:
        norm = torch.nn.utils.clip_grad_norm_(params, max_grad_norm)
    optimizer.step()
    if target_params is not None:
        for target_param, local_param in zip(target_params, params):
            target_param.data.copy_(tau * local_param.data + (1.0 - tau) * target_param.data)
    return norm


class _Table:
    """One ``sgw_adam_step`` call: the tensors of one dtype that stand at one step count, their uploaded plan and the call's buffers."""

    __slots__ = ("params", "step", "pending", "image", "workspace", "out_norm", "norm", "state", "desc")


class FusedAdam(torch.optim.Optimizer):
    """``torch.optim.Adam`` (no weight decay, amsgrad or maximize) with the reference's gradient clipping in front and its soft update
    behind, in one native call per dtype.

    ``params_or_groups``: tensors, or groups with an ``lr`` of their own (PPO's actor and critic are one call); ``betas`` and ``eps`` are
    call-wide.  ``max_grad_norm``: ``clip_grad_norm_(params, max_grad_norm)`` over every gradient first.  ``target_params`` (as many as
    there are parameters, in their order) and ``tau``: ``target = tau * param + (1 - tau) * target`` afterwards.  ``zero_grads``: every
    gradient is set to +0 once it was read.  ``device_step``: the step count and the powers of the betas live on the device (running
    products, not ``pow``), which is what ``torch.cuda.graph`` needs: with stable pointers ``step()`` allocates nothing and can be
    recorded.

    UNLIKE the reference's lines, ``step()`` does not write the clipped gradient back: afterwards ``p.grad`` holds what ``backward``
    left there (or zeros with ``zero_grads``).  ``step()`` returns the gradients' norm as a 0-d float64 tensor when ``max_grad_norm`` is
    given (a view of a buffer the next call overwrites), else None; it never synchronises.  The table of pointers is rebuilt and uploaded
    only when a ``data_ptr`` or a learning rate in it changes.  ``state_dict()`` / ``load_state_dict()`` use ``torch.optim.Adam``'s
    format.  CPU tensors take ``_adam_step_torch``."""

    def __init__(self, params_or_groups, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, *, max_grad_norm=None, target_params=None, tau=None,
                 zero_grads=False, device_step=False):
        beta1, beta2 = (float(b) for b in betas)
        if not (math.isfinite(lr) and math.isfinite(eps)):
            raise ValueError(f"FusedAdam: lr = {lr} and eps = {eps} must be finite")
        if not (0.0 <= beta1 < 1.0 and 0.0 <= beta2 < 1.0):
            raise ValueError(f"FusedAdam: betas = {betas} outside [0, 1)")
        if 1.0 - beta1 >= 0.5:
            raise ValueError(f"FusedAdam: 1 - beta1 = {1.0 - beta1} must be below 0.5")
        if max_grad_norm is not None and not math.isfinite(float(max_grad_norm)):
            raise ValueError(f"FusedAdam: max_grad_norm = {max_grad_norm} must be finite")
        if (target_params is None) != (tau is None):
            raise ValueError("FusedAdam: target_params and tau go together")
        if tau is not None and not math.isfinite(float(tau)):
            raise ValueError(f"FusedAdam: tau = {tau} must be finite")
        defaults = dict(lr=lr, betas=(beta1, beta2), eps=eps, weight_decay=0, amsgrad=False, maximize=False, foreach=None, capturable=False,
                        differentiable=False, fused=None, decoupled_weight_decay=False)
        super().__init__(params_or_groups, defaults)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.tau = None if tau is None else float(tau)
        self.zero_grads, self.device_step = bool(zero_grads), bool(device_step)
        flat = self._flat()
        for p in flat:
            if p.dtype not in _DTYPES:
                raise TypeError(f"FusedAdam: a parameter is {p.dtype}; float32 and float64 are supported")
        self._targets = None
        if target_params is not None:
            targets = list(target_params)
            if len(targets) != len(flat):
                raise ValueError(f"FusedAdam: {len(targets)} target_params for {len(flat)} parameters")
            for p, t in zip(flat, targets):
                if t.shape != p.shape or t.dtype != p.dtype or t.device != p.device:
                    raise ValueError("FusedAdam: a target differs from its parameter in shape, dtype or device")
            self._targets = {id(p): t for p, t in zip(flat, targets)}
        self._key, self._tables, self._inner = None, [], None

    def _flat(self):
        return [p for g in self.param_groups for p in g["params"]]

    def zero_grad(self, set_to_none: bool = False) -> None:
        super().zero_grad(set_to_none=set_to_none)

    # ------------------------------------------------------------------------------------------------------------- Adam's state format
    def _flush(self) -> None:
        """Bring every ``state[p]['step']`` up to date with the calls made since the tables were built."""
        for tb in self._tables:
            if tb.state is not None:
                step = int(tb.state.cpu().view(torch.int64)[0])
            else:
                step = tb.step
            if tb.pending or tb.state is not None:
                for p in tb.params:
                    self.state[p]["step"] = torch.tensor(float(step), dtype=torch.float32)
            tb.pending = 0
            tb.step = step

    def count_on_device(self, on: bool = True) -> None:
        """Switch ``device_step``: the count so far is flushed into ``state[p]['step']`` and the tables are dropped, so the next ``step()`` rebuilds
        them (an upload: not inside a capture) and goes on from the same count.  (The bias corrections then come from running products of the
        betas, not ``pow``: the bits differ from the default's in the last place.)"""
        if bool(on) != self.device_step:
            self._flush()
            self.device_step = bool(on)
            self._key, self._tables = None, []

    def state_dict(self):
        self._flush()
        return super().state_dict()

    def load_state_dict(self, state_dict) -> None:
        super().load_state_dict(state_dict)
        self._key, self._tables = None, []

    # ------------------------------------------------------------------------------------------------------------- the step
    def _hyper(self):
        groups = self.param_groups
        betas, eps = groups[0]["betas"], groups[0]["eps"]
        for g in groups:
            if tuple(g["betas"]) != tuple(betas) or g["eps"] != eps:
                raise ValueError("FusedAdam: betas and eps are call-wide; the groups differ in them")
            if g["weight_decay"] != 0 or g["amsgrad"] or g["maximize"]:
                raise ValueError("FusedAdam: weight decay, amsgrad and maximize are out of scope")
        return float(betas[0]), float(betas[1]), float(eps)

    def _table_key(self, active):
        targets = self._targets
        return tuple((p.data_ptr(), p.grad.data_ptr(), targets[id(p)].data_ptr() if targets else 0, lr) for p, lr in active)

    def table_key(self):
        """What the uploaded table was built from, computed from the tensors as they lie now: ``step()`` rebuilds when it differs."""
        return self._table_key([(p, float(g["lr"])) for g in self.param_groups for p in g["params"] if p.grad is not None])

    @torch.no_grad()
    def step(self, closure=None):
        if closure is not None:
            raise ValueError("FusedAdam.step takes no closure")
        active = [(p, float(g["lr"])) for g in self.param_groups for p in g["params"] if p.grad is not None]
        if not active:
            return None
        devices = {p.device.type for p, _ in active}
        if devices == {"cpu"}:
            return self._step_torch([p for p, _ in active])
        if devices != {"cuda"}:
            raise ValueError(f"FusedAdam: the parameters lie on {sorted(devices)}; one call takes CPU tensors or device tensors")
        key = self._table_key(active)
        if key != self._key:
            self._build(active)
            self._key = key
        from sorrel_amd import _native as N

        for tb in self._tables:
            tb.desc.step = 0 if tb.state is not None else tb.step + 1
            N.launch("sgw_adam_step", tb.desc, active[0][0].device)
            tb.step += 1
            tb.pending += 1
        return self._tables[0].norm if self.max_grad_norm is not None else None

    def _step_torch(self, params):
        self._flush()
        self._key, self._tables = None, []
        if self._inner is None:
            self._inner = torch.optim.Adam(self.param_groups)
        self._inner.param_groups, self._inner.state = self.param_groups, self.state
        self._hyper()
        targets = [self._targets[id(p)] for p in params] if self._targets else None
        norm = _adam_step_torch(params, self._inner, self.max_grad_norm, targets, self.tau)
        if self.zero_grads:
            for p in params:
                p.grad.zero_()
        return None if norm is None else norm.to(torch.float64)

    def _build(self, active) -> None:
        """Group the tensors that have a gradient by dtype and step count, plan every group and upload its table."""
        from sorrel_amd import _native as N

        self._flush()
        beta1, beta2, eps = self._hyper()
        lib, dev = N.load(), active[0][0].device
        groups = {}
        for p, lr in active:
            if p.device != dev:
                raise ValueError(f"FusedAdam: parameters on {dev} and on {p.device}")
            st = self.state[p]
            if len(st) == 0:
                st["step"] = torch.tensor(0.0, dtype=torch.float32)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            t = self._targets[id(p)] if self._targets else None
            for name, x in (("parameter", p), ("gradient", p.grad), ("exp_avg", st["exp_avg"]), ("exp_avg_sq", st["exp_avg_sq"]), ("target", t)):
                if x is None:
                    continue
                if x.dtype != p.dtype or x.device != p.device or x.shape != p.shape:
                    raise ValueError(f"FusedAdam: a {name} differs from its parameter in dtype, device or shape")
                if not x.is_contiguous():
                    raise ValueError(f"FusedAdam: a {name} is not contiguous (strided tensors are out of scope)")
            groups.setdefault((p.dtype, int(st["step"])), []).append((p, lr, t))
        if self.max_grad_norm is not None and len(groups) > 1:
            raise ValueError("FusedAdam: max_grad_norm needs every parameter to share one dtype and one step count "
                             f"(found {sorted((str(d), s) for d, s in groups)})")
        tables = []
        for (dtype, step), members in groups.items():
            if len(members) > N.ADAM_MAX_TENSORS:
                raise ValueError(f"FusedAdam: {len(members)} tensors in one call; at most {N.ADAM_MAX_TENSORS}")
            T = len(members)
            recs = (N.SgwAdamTensor * T)()
            for r, (p, lr, t) in zip(recs, members):
                st = self.state[p]
                r.param, r.grad, r.exp_avg, r.exp_avg_sq = p.data_ptr(), p.grad.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr()
                r.target = t.data_ptr() if t is not None else None
                r.numel, r.lr = p.numel(), lr
            code = N.float_code(dtype)
            size = lib.sgw_adam_plan_bytes(T, sum(p.numel() for p, _, _ in members))
            if size < 0:
                N.check(int(size))
            host = np.zeros((size + 7) // 8, np.int64)
            info = N.SgwAdamPlanInfo()
            N.check(lib.sgw_adam_plan(recs, T, code, host.ctypes.data, host.nbytes, C.byref(info)))
            tb = _Table()
            tb.params, tb.step, tb.pending = [p for p, _, _ in members], step, 0
            tb.image = torch.from_numpy(host).to(dev)
            tb.workspace = N.workspace(info.workspace_bytes, dev)
            tb.out_norm = torch.zeros((2,), dtype=torch.float64, device=dev)
            tb.norm = tb.out_norm[0]
            tb.state = None
            if self.device_step:
                b1p = b2p = 1.0
                for _ in range(step):
                    b1p, b2p = b1p * beta1, b2p * beta2
                cpu = torch.tensor([0.0, b1p, b2p], dtype=torch.float64)
                cpu.view(torch.int64)[0] = step
                tb.state = cpu.to(dev)
            d = N.SgwAdamStepDesc()
            d.plan, d.plan_bytes = tb.image.data_ptr(), info.image_bytes
            d.step_state = tb.state.data_ptr() if tb.state is not None else None
            d.out_norm = tb.out_norm.data_ptr()
            d.workspace, d.workspace_bytes = tb.workspace.data_ptr(), tb.workspace.numel() * 8
            d.num_tensors, d.num_chunks = T, info.num_chunks
            d.max_norm = self.max_grad_norm if self.max_grad_norm is not None else 0.0
            d.beta1, d.beta2, d.eps, d.tau = beta1, beta2, eps, self.tau if self.tau is not None else 0.0
            d.dtype = code
            d.clip_mode = N.ADAM_CLIP_NORM if self.max_grad_norm is not None else N.ADAM_CLIP_NONE
            d.flags = N.ADAM_ZERO_GRADS if self.zero_grads else 0
            tb.desc = d
            tables.append(tb)
        self._tables = tables
