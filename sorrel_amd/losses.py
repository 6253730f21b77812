"""The learners' loss heads on the device.

PPO's clipped loss (``sorrel/models/pytorch/ppo.py:259-285``: the body of ``PyTorchPPO.train_step``'s ``k_epochs`` loop
between the networks' outputs and ``optimizer.step``).

``ppo_loss_terms`` is one ``sgw_ppo_loss`` call (``sorrel_amd/csrc/ppo_loss.h``): it reads each row once and writes the loss terms and
the gradients of the mean loss at the actor's and the critic's outputs.  ``ppo_loss`` wraps it as a ``torch.autograd.Function`` whose
``backward`` hands those gradients on, so a user's learner writes::

    loss = ppo_loss(ActionProbs(actor(states)), critic(states).squeeze(-1), actions, old_log_probs, returns, eps_clip, entropy_coef)
    optimizer.zero_grad(); loss.backward(); optimizer.step()

``_ppo_loss_torch`` is the reference's lines restated with torch ops: the path of CPU tensors, and what the kernel is compared with and
timed against.  Device tensors always use the kernel.  The networks, the optimiser and the learner class stay the user's.

IQN's quantile Huber loss (``sorrel/models/pytorch/iqn.py:359-405``: the body of ``iRainbowModel.train_step`` between the three network
outputs and ``loss.backward()``) has the same three forms -- ``iqn_loss_terms`` (one ``sgw_iqn_loss`` call, ``sorrel_amd/csrc/iqn_loss.h``),
``iqn_loss`` and ``_iqn_loss_torch`` -- so a user's learner writes::

    states, actions, rewards, next_states, dones, valid = buffer.sample(batch_size)
    q_next_local, _ = local(next_states, n_quantiles); q_next_target, _ = target(next_states, n_quantiles)
    q_expected, taus = local(states, n_quantiles)
    loss = iqn_loss(q_expected, taus, q_next_local, q_next_target, actions, rewards, dones, valid, GAMMA ** n_step)
    optimizer.zero_grad(); loss.backward(); clip_grad_norm_(local.parameters(), 1); optimizer.step()
    # or, with optimizer = sorrel_amd.optim.FusedAdam(local.parameters(), max_grad_norm=1, target_params=target.parameters(), tau=TAU): optimizer.step() alone

With ``sorrel_amd.models.iqn.IQN`` the three network calls run without torch's network ops as well (``sgw_iqn_forward``, and
``sgw_iqn_backward`` behind ``loss.backward()``)::

    q_next_local = local.quantiles(next_states).quantiles; q_next_target = target.quantiles(next_states).quantiles
    q_expected, taus = local.forward_fused(states)
    loss = iqn_loss(q_expected, taus, q_next_local, q_next_target, actions, rewards, dones, valid, GAMMA ** n_step); loss.backward(); optimizer.step()

``sorrel_amd.models.PyTorchIQN`` (``models/iqn_learner.py``) is the learner class over these calls: its ``train_step()`` is this step without autograd.
"""
from __future__ import annotations

import torch

from sorrel_amd import _native as N
from sorrel_amd._check import check_tensors
from sorrel_amd.models.base_model import ActionProbs

_FLOATS = (torch.float32, torch.float64)


class PPOLoss:
    """What ``ppo_loss_terms`` gives back: ``loss`` = ``policy + value_coef * value - entropy_coef * entropy``, the three means (0-d
    float64 tensors, views of ``terms`` = ``[L, Pm, M, Hm]``), ``grad_dist`` (dL/d dist: the shape, dtype and strides of the
    distribution's tensor) and ``grad_values`` (dL/d values), and ``row_terms`` (float64 ``[n, 3]`` = per-row policy term, squared
    error and entropy) if asked for, else None.  Passed back as ``out=`` its tensors are overwritten in place."""

    __slots__ = ("terms", "loss", "policy", "value", "entropy", "grad_dist", "grad_values", "row_terms", "_workspace")

    def __init__(self, dist, values, row_terms=False):
        dev, n = dist.device, int(dist.shape[0])
        self.terms = torch.empty((4,), dtype=torch.float64, device=dev)
        self.loss, self.policy, self.value, self.entropy = self.terms[0], self.terms[1], self.terms[2], self.terms[3]
        self.grad_dist = torch.empty_strided(dist.shape, dist.stride(), dtype=dist.dtype, device=dev)
        self.grad_values = torch.empty(values.shape, dtype=values.dtype, device=dev)
        self.row_terms = torch.empty((n, 3), dtype=torch.float64, device=dev) if row_terms else None
        self._workspace = None
        if dev.type == "cuda":
            self._workspace = N.workspace(N.load().sgw_ppo_loss_workspace_bytes(n), dev)

    def __repr__(self):
        return f"PPOLoss(n={self.grad_values.numel()}, num_actions={self.grad_dist.shape[1]})"


def _unwrap(dist):
    """``(tensor, logits)`` of an ``ActionProbs`` / ``ActionLogits``, or of a bare 2-D tensor taken as probabilities."""
    if isinstance(dist, ActionProbs):
        return dist.tensor, bool(dist.logits)
    return ActionProbs(dist).tensor, False


def _check(t, values, actions, old_log_probs, returns):
    n, na = int(t.shape[0]), int(t.shape[1])
    if t.stride(1) != 1 and na > 1 or (n > 1 and t.stride(0) < na):
        raise ValueError(f"the distribution's rows must be contiguous (strides {tuple(t.stride())})")
    check_tensors(t.device, "the distribution", ("values", values, _FLOATS, n), ("actions", actions, (torch.int64, torch.uint8), n),
                  ("old_log_probs", old_log_probs, (torch.float32,), n), ("returns", returns, _FLOATS, n))
    return n, na


def _check_out(out, t, values, row_terms):
    if not isinstance(out, PPOLoss):
        raise TypeError("out= takes an earlier PPOLoss")
    n = int(t.shape[0])
    tensors = [out.terms, out.grad_dist, out.grad_values] + [x for x in (out.row_terms, out._workspace) if x is not None]
    if (out.grad_dist.shape != t.shape or out.grad_dist.stride() != t.stride() or out.grad_dist.dtype != t.dtype
            or out.grad_values.shape != values.shape or out.grad_values.dtype != values.dtype
            or any(x.device != t.device for x in tensors)
            or (row_terms and (out.row_terms is None or tuple(out.row_terms.shape) != (n, 3)))
            or (t.device.type == "cuda" and out._workspace is None)):
        raise ValueError("out= was made for other shapes, strides, dtypes or another device")
    return out


def _ppo_loss_torch(t, logits, values, actions, old_log_probs, returns, eps_clip, entropy_coef, value_coef=0.5):
    """The reference's lines (``ppo.py:152-158`` and ``:265-284``) with torch ops, in float64 as its ``ActorCritic`` runs: returns
    ``(loss.mean(), policy_loss.mean(), critic_loss, dist_entropy.mean(), policy_loss, squared errors, dist_entropy)``, connected to
    ``t`` and ``values`` for autograd.  ``Categorical`` skips its argument check (a host synchronisation the timed baseline is
    spared), so an invalid row is not refused here."""
    from torch.distributions import Categorical

    n = t.shape[0]
    x = t.double()
    dist = Categorical(logits=x, validate_args=False) if logits else Categorical(probs=x, validate_args=False)
    acts = actions.reshape(n).long()
    log_probs = dist.log_prob(acts)
    dist_entropy = dist.entropy()
    state_values = values.reshape(n).double()
    rewards = returns.reshape(n).double()
    ratios = torch.exp(log_probs - old_log_probs.reshape(n).double().detach())
    advantages = rewards - state_values.detach()
    surr1 = ratios * advantages
    surr2 = torch.clamp(ratios, 1 - eps_clip, 1 + eps_clip) * advantages
    sq = (state_values - rewards) ** 2
    critic_loss = sq.mean()                                 # nn.MSELoss()(state_values, rewards)
    policy_loss = -torch.min(surr1, surr2)
    loss = policy_loss + value_coef * critic_loss - entropy_coef * dist_entropy
    return loss.mean(), policy_loss.mean(), critic_loss, dist_entropy.mean(), policy_loss, sq, dist_entropy


def _terms_by_torch(t, logits, values, actions, old_log_probs, returns, eps_clip, entropy_coef, value_coef, res):
    with torch.enable_grad():
        leaf_t, leaf_v = t.detach().requires_grad_(True), values.detach().requires_grad_(True)
        L, Pm, M, Hm, P, sq, H = _ppo_loss_torch(leaf_t, logits, leaf_v, actions, old_log_probs, returns, eps_clip, entropy_coef, value_coef)
        g_t, g_v = torch.autograd.grad(L, (leaf_t, leaf_v))
    res.terms.copy_(torch.stack((L, Pm, M, Hm)).detach())
    res.grad_dist.copy_(g_t)
    res.grad_values.copy_(g_v)
    if res.row_terms is not None:
        res.row_terms.copy_(torch.stack((P, sq, H), dim=1).detach())
    return res


def ppo_loss_terms(dist, values, actions, old_log_probs, returns, eps_clip, entropy_coef, value_coef=0.5, *, out=None, row_terms=False):
    """The clipped PPO loss of ``n`` rows and its gradients: ``dist`` is an ``ActionProbs`` / ``ActionLogits`` or a bare ``[n, n_actions]``
    tensor of (unnormalised) probabilities, float32 or float64; ``values`` (float32 / float64), ``actions`` (int64 / uint8),
    ``old_log_probs`` (float32: what ``sgw_policy_sample`` stored) and ``returns`` (float32 / float64: ``Returns.normalized`` or
    ``.returns``) have any leading shape with ``n`` elements -- a ring segment ``[count, E]`` with ``dist`` its ``[count * E, A]`` view --
    and are contiguous.  Returns a ``PPOLoss``.  On a HIP device this is one ``sgw_ppo_loss`` call in float64 whatever the inputs'
    types; with ``out=`` (an earlier result for the same shapes) it allocates nothing and does not synchronise, so it can be recorded
    into a graph.  A row ``Categorical`` would refuse, or whose action is out of range, gives NaN for its outputs and for the means."""
    t, logits = _unwrap(dist)
    if not torch.is_tensor(values):
        raise TypeError(f"values must be a tensor, not {type(values).__name__}")
    n, na = _check(t, values, actions, old_log_probs, returns)
    eps_clip, entropy_coef, value_coef = float(eps_clip), float(entropy_coef), float(value_coef)
    if not (eps_clip >= 0.0 and eps_clip != float("inf")):
        raise ValueError(f"eps_clip = {eps_clip} must be finite and not negative")
    res = PPOLoss(t, values, row_terms) if out is None else _check_out(out, t, values, row_terms)
    if t.device.type != "cuda":
        return _terms_by_torch(t, logits, values, actions, old_log_probs, returns, eps_clip, entropy_coef, value_coef, res)
    if n == 0:
        res.terms.fill_(float("nan"))                        # the mean of nothing, as torch's
        return res
    d = N.SgwPpoLossDesc()
    d.dist, d.values, d.actions, d.old_log_probs, d.returns = t.data_ptr(), values.data_ptr(), actions.data_ptr(), old_log_probs.data_ptr(), returns.data_ptr()
    d.out_grad_dist, d.out_grad_values, d.out_terms = res.grad_dist.data_ptr(), res.grad_values.data_ptr(), res.terms.data_ptr()
    if row_terms:
        d.out_row_terms = res.row_terms.data_ptr()
    d.workspace, d.workspace_bytes = res._workspace.data_ptr(), res._workspace.numel() * 8
    d.n, d.row_stride, d.num_actions = n, (int(t.stride(0)) if n > 1 else na), na
    d.eps_clip, d.entropy_coef, d.value_coef = eps_clip, entropy_coef, value_coef
    d.dist_type, d.mode = N.float_code(t.dtype), (N.POLICY_LOGITS if logits else N.POLICY_PROBS)
    d.value_type, d.returns_type, d.action_type = N.float_code(values.dtype), N.float_code(returns.dtype), N.action_code(actions.dtype)
    N.launch("sgw_ppo_loss", d, t.device)
    return res


class _PPOLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t, values, logits, actions, old_log_probs, returns, eps_clip, entropy_coef, value_coef, out):
        from sorrel_amd.models.base_model import ActionLogits

        res = ppo_loss_terms((ActionLogits if logits else ActionProbs)(t.detach()), values.detach(), actions, old_log_probs, returns,
                             eps_clip, entropy_coef, value_coef, out=out)
        ctx.save_for_backward(res.grad_dist, res.grad_values)
        return res.loss.clone()

    @staticmethod
    def backward(ctx, grad_out):
        g_t, g_v = ctx.saved_tensors
        # one multiply per gradient: the incoming gradient is a device scalar (1 after loss.backward()) and is not read on the host
        return (g_t * grad_out.to(g_t.dtype) if ctx.needs_input_grad[0] else None, g_v * grad_out.to(g_v.dtype) if ctx.needs_input_grad[1] else None,
                None, None, None, None, None, None, None, None)


def ppo_loss(dist, values, actions, old_log_probs, returns, eps_clip, entropy_coef, value_coef=0.5, *, out=None):
    """``ppo_loss_terms`` as a differentiable scalar: the loss ``L`` (0-d float64), connected to the distribution's tensor and to
    ``values``.  The forward launch has already written both gradients; ``backward`` multiplies them by the incoming gradient and hands
    them on to the networks.  ``out=``: a ``PPOLoss`` to reuse (it must not be overwritten before ``backward`` ran)."""
    t, logits = _unwrap(dist)
    if not torch.is_tensor(values):
        raise TypeError(f"values must be a tensor, not {type(values).__name__}")
    return _PPOLossFn.apply(t, values, logits, actions, old_log_probs, returns, eps_clip, entropy_coef, value_coef, out)


# ---------------------------------------------------------------------------------------------------------------- IQN's quantile Huber loss
class IQNLoss:
    """What ``iqn_loss_terms`` gives back: ``loss`` (0-d float64, a view of ``terms`` = ``[L]``), ``grad_expected`` (dL/d q_expected,
    float32 ``[B, N, A]``, every element written), ``next_actions`` (int64 ``[B]``: the double-DQN choice ``a*``), and, if asked for,
    ``row_terms`` (float64 ``[B]``: the rows' sums ``S_b``) and ``td_error`` (float32 ``[B, N, N]``: what a prioritised replay needs),
    else None.  Passed back as ``out=`` its tensors are overwritten in place."""

    __slots__ = ("terms", "loss", "grad_expected", "next_actions", "row_terms", "td_error", "_workspace")

    def __init__(self, q_expected, row_terms=False, td_error=False):
        dev = q_expected.device
        B, Nq, _A = (int(s) for s in q_expected.shape)
        self.terms = torch.empty((1,), dtype=torch.float64, device=dev)
        self.loss = self.terms[0]
        self.grad_expected = torch.empty(q_expected.shape, dtype=torch.float32, device=dev)
        self.next_actions = torch.empty((B,), dtype=torch.int64, device=dev)
        self.row_terms = torch.empty((B,), dtype=torch.float64, device=dev) if row_terms else None
        self.td_error = torch.empty((B, Nq, Nq), dtype=torch.float32, device=dev) if td_error else None
        self._workspace = None
        if dev.type == "cuda":
            self._workspace = N.workspace(N.load().sgw_iqn_loss_workspace_bytes(B, Nq), dev)

    def __repr__(self):
        return f"IQNLoss(n={self.grad_expected.shape[0]}, num_quantiles={self.grad_expected.shape[1]}, num_actions={self.grad_expected.shape[2]})"


def _check_iqn(q_expected, taus, q_next_local, q_next_target, actions, rewards, dones, valid):
    for name, x in (("q_expected", q_expected), ("taus", taus), ("q_next_local", q_next_local), ("q_next_target", q_next_target),
                    ("actions", actions), ("rewards", rewards), ("dones", dones), ("valid", valid)):
        if not torch.is_tensor(x):
            raise TypeError(f"{name} must be a tensor, not {type(x).__name__}")
    if q_expected.dim() != 3:
        raise ValueError(f"q_expected must be [B, N, A], not {tuple(q_expected.shape)}")
    B, Nq, A = (int(s) for s in q_expected.shape)
    if not 1 <= Nq <= N.IQN_MAX_QUANTILES:
        raise ValueError(f"{Nq} quantiles: the loss takes 1..{N.IQN_MAX_QUANTILES}")
    if not 1 <= A <= N.POLICY_MAX_ACTIONS:
        raise ValueError(f"{A} actions: the loss takes 1..{N.POLICY_MAX_ACTIONS}")
    f32 = (torch.float32,)
    full, row = ((B, Nq, A),), ((B, 1), (B,))
    check_tensors(q_expected.device, "q_expected",
                  ("q_expected", q_expected, f32, full), ("q_next_local", q_next_local, f32, full), ("q_next_target", q_next_target, f32, full),
                  ("taus", taus, f32, ((B, Nq, 1), (B, Nq))), ("actions", actions, (torch.int64, torch.uint8), row), ("rewards", rewards, f32, row),
                  ("dones", dones, f32, row), ("valid", valid, _FLOATS, row))
    return B, Nq, A


def _check_iqn_out(out, q_expected, row_terms, td_error):
    if not isinstance(out, IQNLoss):
        raise TypeError("out= takes an earlier IQNLoss")
    tensors = [out.terms, out.grad_expected, out.next_actions] + [x for x in (out.row_terms, out.td_error, out._workspace) if x is not None]
    if (out.grad_expected.shape != q_expected.shape or any(x.device != q_expected.device for x in tensors)
            or (row_terms and out.row_terms is None) or (td_error and out.td_error is None)
            or (q_expected.device.type == "cuda" and out._workspace is None)):
        raise ValueError("out= was made for other shapes or another device, or without the optional outputs asked for")
    return out


def _iqn_loss_torch(q_expected, taus, q_next_local, q_next_target, actions, rewards, dones, valid, discount):
    """The reference's lines (``iqn.py:359-402`` and ``calculate_huber_loss``) with torch ops: returns ``(loss, td_error, action_indx,
    quantil_l)``, connected to ``q_expected`` for autograd.  ``discount`` is ``GAMMA ** n_step``."""
    B, N, _A = q_expected.shape
    actions, rewards, dones, valid = actions.reshape(B, 1).long(), rewards.reshape(B, 1), dones.reshape(B, 1), valid.reshape(B, 1)
    taus = taus.reshape(B, N, 1)
    action_indx = torch.argmax(q_next_local.detach().mean(dim=1), dim=1, keepdim=True)
    Q_targets_next = q_next_target.detach().gather(2, action_indx.unsqueeze(-1).expand(B, N, 1)).transpose(1, 2)
    Q_targets = rewards.unsqueeze(-1) + (discount * Q_targets_next * (1.0 - dones.unsqueeze(-1)))
    Q_expected = q_expected.gather(2, actions.unsqueeze(-1).expand(B, N, 1))
    td_error = Q_targets - Q_expected
    huber_l = torch.where(td_error.abs() <= 1.0, 0.5 * td_error.pow(2), 1.0 * (td_error.abs() - 0.5 * 1.0))
    huber_l = huber_l * valid.unsqueeze(-1)
    quantil_l = abs(taus.detach() - (td_error.detach() < 0).float()) * huber_l / 1.0
    return quantil_l.mean(), td_error, action_indx.reshape(B), quantil_l


def _iqn_terms_by_torch(q_expected, taus, q_next_local, q_next_target, actions, rewards, dones, valid, discount, res):
    with torch.enable_grad():
        leaf = q_expected.detach().requires_grad_(True)
        L, td, a_star, ql = _iqn_loss_torch(leaf, taus, q_next_local, q_next_target, actions, rewards, dones, valid, discount)
        (g,) = torch.autograd.grad(L, (leaf,))
    res.terms.copy_(L.detach().double().reshape(1))
    res.grad_expected.copy_(g)
    res.next_actions.copy_(a_star)
    if res.row_terms is not None:
        res.row_terms.copy_(ql.detach().double().sum(dim=(1, 2)))
    if res.td_error is not None:
        res.td_error.copy_(td.detach())
    return res


def iqn_loss_terms(q_expected, taus, q_next_local, q_next_target, actions, rewards, dones, valid, discount, *, out=None, row_terms=False,
                   td_error=False):
    """IQN's quantile Huber loss (kappa = 1) of a batch and its gradient at ``q_expected``: the three quantile tensors are contiguous
    float32 ``[B, N, A]`` (the local net on the states, and the local and the target net on the next states), ``taus`` float32
    ``[B, N, 1]`` or ``[B, N]`` (the taus of the ``q_expected`` call), ``actions`` (int64 / uint8), ``rewards``, ``dones`` (float32) and
    ``valid`` (float32 / float64, any row weight) ``[B, 1]`` or ``[B]`` -- what ``Buffer.sample`` and ``TurnBuffer.sample`` hand over --
    and ``discount`` is ``GAMMA ** n_step``.  Returns an ``IQNLoss``.  On a HIP device this is one ``sgw_iqn_loss`` call; with ``out=``
    (an earlier result for the same shapes) it allocates nothing and does not synchronise, so it can be recorded into a graph.  A row
    whose action is out of range gives NaN for its term, its gradient row and the loss."""
    B, Nq, A = _check_iqn(q_expected, taus, q_next_local, q_next_target, actions, rewards, dones, valid)
    discount = float(discount)
    if discount != discount or discount in (float("inf"), float("-inf")):
        raise ValueError(f"discount = {discount} must be finite")
    res = IQNLoss(q_expected, row_terms, td_error) if out is None else _check_iqn_out(out, q_expected, row_terms, td_error)
    if q_expected.device.type != "cuda":
        return _iqn_terms_by_torch(q_expected, taus, q_next_local, q_next_target, actions, rewards, dones, valid, discount, res)
    if B == 0:
        res.terms.fill_(float("nan"))                        # the mean of nothing, as torch's
        return res
    d = N.SgwIqnLossDesc()
    d.q_next_local, d.q_next_target, d.q_expected, d.taus = q_next_local.data_ptr(), q_next_target.data_ptr(), q_expected.data_ptr(), taus.data_ptr()
    d.actions, d.rewards, d.dones, d.valid = actions.data_ptr(), rewards.data_ptr(), dones.data_ptr(), valid.data_ptr()
    d.out_terms, d.out_grad_expected, d.out_next_actions = res.terms.data_ptr(), res.grad_expected.data_ptr(), res.next_actions.data_ptr()
    if row_terms:
        d.out_row_terms = res.row_terms.data_ptr()
    if td_error:
        d.out_td_error = res.td_error.data_ptr()
    d.workspace, d.workspace_bytes = res._workspace.data_ptr(), res._workspace.numel() * 8
    d.n, d.num_quantiles, d.num_actions, d.discount = B, Nq, A, discount
    d.action_type, d.valid_type = N.action_code(actions.dtype), N.float_code(valid.dtype)
    N.launch("sgw_iqn_loss", d, q_expected.device)
    return res


class _IQNLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q_expected, taus, q_next_local, q_next_target, actions, rewards, dones, valid, discount, out):
        res = iqn_loss_terms(q_expected.detach(), taus.detach(), q_next_local.detach(), q_next_target.detach(), actions, rewards, dones, valid,
                             discount, out=out)
        ctx.save_for_backward(res.grad_expected)
        return res.loss.clone()

    @staticmethod
    def backward(ctx, grad_out):
        (g,) = ctx.saved_tensors
        # one multiply: the incoming gradient is a device scalar (1 after loss.backward()) and is not read on the host
        return (g * grad_out.to(g.dtype) if ctx.needs_input_grad[0] else None,) + (None,) * 9


def iqn_loss(q_expected, taus, q_next_local, q_next_target, actions, rewards, dones, valid, discount, *, out=None):
    """``iqn_loss_terms`` as a differentiable scalar: the loss ``L`` (0-d float64), connected to ``q_expected`` only (nothing flows to
    ``taus`` or to the next states' quantiles, as in the reference).  The forward launch has already written the gradient; ``backward``
    multiplies it by the incoming gradient and hands it on.  ``out=``: an ``IQNLoss`` to reuse (it must not be overwritten before
    ``backward`` ran)."""
    for name, x in (("q_expected", q_expected), ("taus", taus), ("q_next_local", q_next_local), ("q_next_target", q_next_target)):
        if not torch.is_tensor(x):
            raise TypeError(f"{name} must be a tensor, not {type(x).__name__}")
    return _IQNLossFn.apply(q_expected, taus, q_next_local, q_next_target, actions, rewards, dones, valid, discount, out)
