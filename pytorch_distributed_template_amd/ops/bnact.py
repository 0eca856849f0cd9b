"""Training-mode BatchNorm fused with the activation behind it on the native HIP kernels (``csrc/kernels/bnact.hip``).

Functional ops (the unit-test surface, tests/test_bnact_gpu.py) over NHWC 16-bit activations viewed as ``[rows, C]``
with ``C % 8 == 0`` and ``C <= MAX_C``; ``act`` is one of :data:`ACTS`:

* :func:`bnact_stats`       per-channel statistics -> ``coef = [scale | shift | mean | invstd]`` (+ running statistics)
* :func:`bnact_fwd`         ``out = act(x * scale + shift)``
* :func:`bnact_bwd_reduce`  fp64 ``[sum dz | sum dz * xhat]`` with ``dz = g * act'(x * scale + shift)`` recomputed
* :func:`bnact_bwd_apply`   ``dx = A * dz + B * x + Cc``

and the drop-in module for the torch engine:

* :class:`BNAct2d`       an ``nn.BatchNorm2d`` with an ``act`` that runs the kernels on 16-bit ``channels_last`` GPU
  inputs in training mode (the torch engine's training activations under autocast) and ``act(BatchNorm2d(x))`` on
  stock ops otherwise
* :func:`convert_bnact`  swaps every qualifying ``nn.BatchNorm2d`` of a model in place and absorbs the activation that
  follows it inside an ``nn.Sequential`` (``--native-bnact on``)
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import native

ACTS = ("identity", "relu", "relu6", "hardswish")  # the kernels' activation codes are the indices
MAX_C = 2048

_DTYPES = (torch.bfloat16, torch.float16)
_ACT_FN = {"identity": lambda t: t, "relu": F.relu, "relu6": F.relu6, "hardswish": F.hardswish}
_ACT_OF = {nn.ReLU: "relu", nn.ReLU6: "relu6", nn.Hardswish: "hardswish"}


def _slots(C: int, device) -> torch.Tensor:
    return torch.empty(native.C.stat_slots() * C * 2, dtype=torch.float64, device=device)


def bnact_stats(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, running_mean: torch.Tensor,
                running_var: torch.Tensor, eps: float, momentum: float, update_running: bool = True) -> torch.Tensor:
    """``coef[4 * C]`` (fp32) of ``x[..., C]`` (NHWC contiguous, 16-bit); updates the running statistics in place."""
    C = x.shape[-1]
    rows = x.numel() // C
    slots = _slots(C, x.device)
    native.C.bnact_stats(x, slots, rows, C)
    return bnact_coef_from_slots(slots, rows, gamma, beta, running_mean, running_var, eps, momentum, update_running)


def bnact_coef_from_slots(slots: torch.Tensor, rows: int, gamma: torch.Tensor, beta: torch.Tensor,
                          running_mean: torch.Tensor, running_var: torch.Tensor, eps: float, momentum: float,
                          update_running: bool = True) -> torch.Tensor:
    """The finalize half of :func:`bnact_stats`: ``coef[4 * C]`` from fp64 ``slots[stat_slots, C, 2]`` of
    ``(sum x, sum x**2)`` over ``rows`` values per channel, whoever filled them (``bnact_stats`` or the producing conv,
    ``ops.pointwise.pwconv_fwd_stats``); updates the running statistics in place."""
    C = gamma.numel()
    coef = torch.empty(4 * C, dtype=torch.float32, device=slots.device)
    sums = torch.empty(2 * C, dtype=torch.float64, device=slots.device)
    native.C.bn_finalize_slots(slots, float(rows), gamma, beta, eps, momentum, running_mean, running_var, coef, sums,
                               update_running)
    return coef


def bnact_fwd(x: torch.Tensor, coef: torch.Tensor, act: str) -> torch.Tensor:
    C = x.shape[-1]
    out = torch.empty_like(x)
    native.C.bnact_fwd(x, coef, out, x.numel() // C, C, ACTS.index(act))
    return out


def bnact_bwd_reduce(g: torch.Tensor, x: torch.Tensor, coef: torch.Tensor, act: str) -> torch.Tensor:
    """fp64 ``sums[2 * C] = [sum dz | sum dz * xhat]``."""
    C = x.shape[-1]
    slots = _slots(C, x.device)
    native.C.bnact_bwd_reduce(g, x, coef, slots, x.numel() // C, C, ACTS.index(act))
    sums = torch.empty(2 * C, dtype=torch.float64, device=x.device)
    native.C.bn_slot_sum(slots, C, 2, sums)
    return sums


def bnact_bwd_coef(sums: torch.Tensor, rows: int, coef: torch.Tensor, gamma: torch.Tensor):
    """``(dgamma, dbeta, bcoef = [A | B | Cc])`` (fp32) of the backward sums."""
    C = gamma.numel()
    dgamma = torch.empty(C, dtype=torch.float32, device=gamma.device)
    dbeta = torch.empty_like(dgamma)
    bcoef = torch.empty(3 * C, dtype=torch.float32, device=gamma.device)
    native.C.bn_bwd_finalize(sums, float(rows), coef, gamma, dgamma, dbeta, 1.0, bcoef)
    return dgamma, dbeta, bcoef


def bnact_bwd_apply(g: torch.Tensor, x: torch.Tensor, coef: torch.Tensor, bcoef: torch.Tensor, act: str) -> torch.Tensor:
    C = x.shape[-1]
    dx = torch.empty_like(x)
    native.C.bnact_bwd_apply(g, x, coef, bcoef, dx, x.numel() // C, C, ACTS.index(act))
    return dx


# The hand-over of a producing conv's statistics (ops.pointwise.PointwiseConv2d with ``emit_stats``): a plain Python
# attribute ``(slots, version)`` on the very tensor object the conv returned, ``version`` being its ``_version`` then.
CONV_STATS_ATTR = "_pdt_conv_stats"


def take_conv_stats(t: torch.Tensor):
    """Remove and return the ``(slots, version)`` a conv attached to ``t``, or ``None``."""
    return t.__dict__.pop(CONV_STATS_ATTR, None)


def qualifies(m: nn.BatchNorm2d) -> bool:
    """The BatchNorms the kernels cover (everything else stays on ``F.batch_norm``)."""
    return (m.affine and m.track_running_stats and m.momentum is not None and m.num_features % 8 == 0
            and m.num_features <= MAX_C)


class _BNActFn(torch.autograd.Function):
    """``x``: logical NCHW, dense in channels_last, 16-bit; ``gamma`` / ``beta``: the fp32 masters.  Saves ``x`` and the
    per-channel coefficients only: the backward recomputes the pre-activation value from ``x``."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, eps, momentum, act, slots=None):
        xh = x.permute(0, 2, 3, 1)  # NHWC view of the channels_last storage: no copy
        if slots is None:
            coef = bnact_stats(xh, gamma.detach(), beta.detach(), running_mean, running_var, eps, momentum)
        else:  # the statistics of x from the conv that produced it: a non-differentiable extra, same autograd
            coef = bnact_coef_from_slots(slots, xh.numel() // xh.shape[-1], gamma.detach(), beta.detach(),
                                         running_mean, running_var, eps, momentum)
        out = bnact_fwd(xh, coef, act)
        ctx.save_for_backward(x, coef, gamma)
        ctx.act = act
        return out.permute(0, 3, 1, 2)  # channels_last NCHW view

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        x, coef, gamma = ctx.saved_tensors
        xh = x.permute(0, 2, 3, 1)
        g = gy.permute(0, 2, 3, 1)
        if g.dtype != x.dtype or not g.is_contiguous():
            g = g.to(x.dtype).contiguous()
        sums = bnact_bwd_reduce(g, xh, coef, ctx.act)
        dgamma, dbeta, bcoef = bnact_bwd_coef(sums, xh.numel() // xh.shape[-1], coef, gamma.detach())
        dx = None
        if ctx.needs_input_grad[0]:
            dx = bnact_bwd_apply(g, xh, coef, bcoef, ctx.act).permute(0, 3, 1, 2)
        return dx, dgamma, dbeta, None, None, None, None, None, None


class BNAct2d(nn.BatchNorm2d):
    """``nn.BatchNorm2d`` (same constructor plus ``act``, same parameters, buffers and state-dict keys) followed by
    ``act``.  In training mode, a qualifying module runs a 16-bit, dense ``channels_last`` GPU input on the native
    kernels; CPU, fp32, NCHW and eval-mode inputs, non-qualifying configurations and batches with fewer than 2 values
    per channel take ``act(nn.BatchNorm2d.forward(x))`` exactly as the stock modules do."""

    act = "identity"

    def __init__(self, num_features, eps=1e-5, momentum=0.1, affine=True, track_running_stats=True, device=None,
                 dtype=None, act: str = "identity"):
        super().__init__(num_features, eps, momentum, affine, track_running_stats, device=device, dtype=dtype)
        if act not in ACTS:
            raise ValueError(f"act must be one of {ACTS}, got {act!r}")
        self.act = act

    def extra_repr(self) -> str:
        return super().extra_repr() + f", act={self.act}"

    def forward(self, input: torch.Tensor) -> torch.Tensor:
        handed = take_conv_stats(input)  # removed whatever path is taken below
        if (self.training and input.is_cuda and input.dtype in _DTYPES and input.dim() == 4 and qualifies(self)
                and self.weight.dtype == torch.float32 and input.shape[1] == self.num_features
                and input.numel() // self.num_features >= 2
                and input.is_contiguous(memory_format=torch.channels_last)):
            return self._forward_native(input, handed)
        return _ACT_FN[self.act](super().forward(input))

    def _forward_native(self, input: torch.Tensor, handed=None) -> torch.Tensor:
        """The kernels' path.  ``handed``: the ``(slots, version)`` the producing conv attached to this very tensor; the
        slots replace ``bnact_stats`` only if the tensor was not changed in place since and the width is this module's."""
        self.num_batches_tracked.add_(1)
        slots = None
        if (handed is not None and handed[1] == input._version
                and handed[0].numel() == native.C.stat_slots() * self.num_features * 2):
            slots = handed[0]
        return _BNActFn.apply(input, self.weight, self.bias, self.running_mean, self.running_var, self.eps,
                              self.momentum, self.act, slots)


def _as_bnact(bn: nn.BatchNorm2d, act: str) -> BNAct2d:
    # the same module state under the new class: parameters and buffers (the same objects), hooks, training flag
    new = BNAct2d.__new__(BNAct2d)
    new.__dict__ = bn.__dict__.copy()
    for k in ("_parameters", "_buffers", "_modules"):
        new.__dict__[k] = bn.__dict__[k].copy()
    new.__dict__["act"] = act
    return new


def convert_bnact(model: nn.Module):
    """Swap every qualifying ``nn.BatchNorm2d`` below ``model`` for a :class:`BNAct2d` holding the same ``Parameter``
    and buffer objects.  Where the next sibling inside an ``nn.Sequential`` is an ``nn.ReLU``, ``nn.ReLU6`` or
    ``nn.Hardswish``, the BatchNorm absorbs it and the activation module becomes ``nn.Identity()`` (indices and
    state-dict keys stay).  Returns ``(BatchNorms swapped, activations absorbed)``, ``(0, 0)`` on a second call.  Call
    it before the parameters are flattened (``optim.flat.FlatParams``) and not on a model that will be converted to
    SyncBatchNorm."""
    n_bn = n_abs = 0
    for parent in list(model.modules()):
        children = list(parent._modules.items())  # every slot in order (named_children() drops repeated instances)
        sequential = isinstance(parent, nn.Sequential) and type(parent).forward is nn.Sequential.forward
        for i, (name, child) in enumerate(children):
            if not (type(child) is nn.BatchNorm2d and qualifies(child)):
                continue
            act = "identity"
            if sequential and i + 1 < len(children):
                nxt_name, nxt = children[i + 1]
                if type(nxt) in _ACT_OF and not nxt._forward_hooks and not nxt._forward_pre_hooks:
                    act = _ACT_OF[type(nxt)]
                    setattr(parent, nxt_name, nn.Identity())
                    n_abs += 1
            setattr(parent, name, _as_bnact(child, act))
            n_bn += 1
    return n_bn, n_abs
