"""Pointwise (1x1) convolution on the native HIP kernels (``csrc/kernels/pwconv.hip``).

Functional ops (the unit-test surface, tests/test_pointwise_gpu.py) over NHWC 16-bit activations seen as ``[M, C]``
(``M = N * H * W``) and a 16-bit ``[K, C]`` weight, for kernel 1x1, stride 1, padding 0, dilation 1, groups 1, no bias,
``C % 8 == K % 8 == 0`` and ``8 <= C, K <= 2048``:

* :func:`pwconv_fwd`    forward, ``y = x @ w.T``
* :func:`pwconv_fwd_stats`  the same forward plus the BatchNorm statistics (sum, sum of squares) of its rounded output
* :func:`pwconv_dgrad`  gradient w.r.t. the input, ``dx = dy @ w`` (the same kernel on ``w.T``, transposed once here)
* :func:`pwconv_wgrad`  gradient w.r.t. the weight, fp32, deterministic (per-split partial slabs + fixed-order sum)

and the drop-in module for the torch engine:

* :class:`PointwiseConv2d`  an ``nn.Conv2d`` whose forward runs the kernels when the input is a 16-bit
  ``channels_last`` GPU tensor (the torch engine's training activations under autocast) and ``F.conv2d`` otherwise
* :func:`convert_pointwise` swaps every qualifying ``nn.Conv2d`` of a model in place (``--native-pointwise on``)
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import native
from .bnact import CONV_STATS_ATTR

# blocks the weight gradient aims for: a few per CU (256 CUs, two 64 KiB-LDS blocks resident on each)
WGRAD_TARGET_BLOCKS = 1024
MIN_CH, MAX_CH = 8, 2048

_DTYPES = (torch.bfloat16, torch.float16)


def fits(M: int, C: int, K: int) -> bool:
    """The kernels' contract on sizes (widths and the number of rows one launch addresses)."""
    return bool(native.C.pwconv_fits(M, C, K))


def pwconv_fwd(x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """``y[..., K]`` of ``x[..., C]`` (NHWC contiguous, 16-bit) and ``w[K, C]`` (same dtype)."""
    K, C = w.shape
    y = torch.empty(x.shape[:-1] + (K,), dtype=x.dtype, device=x.device)
    native.C.pwconv_fwd(x, w, y, x.numel() // C, C, K)
    return y


def pwconv_fwd_stats(x: torch.Tensor, w: torch.Tensor, max_blocks: int = 0):
    """``(y, slots, (partial_rows, chain))``: ``y`` as :func:`pwconv_fwd` writes it, bit for bit, and the fp64
    ``slots[stat_slots, K, 2]`` holding ``(sum y, sum y**2)`` per channel of the rounded ``y`` -- what
    ``bn_finalize_slots`` (:func:`ops.bnact.bnact_coef_from_slots`) reads, so the BatchNorm behind the conv need not
    read ``y`` again.  ``max_blocks``: persistent blocks the launch aims for (0: the forward's default); ``chain`` is the
    longest run of fp32 additions a statistic passes through before the fp64 sums."""
    K, C = w.shape
    y = torch.empty(x.shape[:-1] + (K,), dtype=x.dtype, device=x.device)
    slots = torch.empty(native.C.stat_slots() * K * 2, dtype=torch.float64, device=x.device)
    rows, chain = native.C.pwconv_fwd_stats(x, w, y, slots, x.numel() // C, C, K, max_blocks)
    return y, slots, (rows, chain)


def pwconv_dgrad(dy: torch.Tensor, w: torch.Tensor, wt: torch.Tensor | None = None) -> torch.Tensor:
    """``dx[..., C]`` of ``dy[..., K]`` and ``w[K, C]``; ``wt``: the contiguous ``[C, K]`` transpose if the caller
    already holds it."""
    K, C = w.shape
    if wt is None:
        wt = w.t().contiguous()
    dx = torch.empty(dy.shape[:-1] + (C,), dtype=dy.dtype, device=dy.device)
    native.C.pwconv_dgrad(dy, wt, dx, dy.numel() // K, C, K)
    return dx


def pwconv_wgrad_plan(M: int, C: int, K: int, target_blocks: int = WGRAD_TARGET_BLOCKS):
    """``(splits, pixels per split, C tiles, K tiles)`` the weight gradient uses for ``M`` pixels."""
    return tuple(native.C.pwconv_wgrad_plan(M, C, K, target_blocks))


def pwconv_wgrad(x: torch.Tensor, dy: torch.Tensor, target_blocks: int = WGRAD_TARGET_BLOCKS) -> torch.Tensor:
    """``dw[K, C]`` (fp32) of ``x[..., C]`` and ``dy[..., K]``."""
    C, K = x.shape[-1], dy.shape[-1]
    M = x.numel() // C
    splits = pwconv_wgrad_plan(M, C, K, target_blocks)[0]
    ws = torch.empty((splits, K, C), dtype=torch.float32, device=x.device)
    got = native.C.pwconv_wgrad(x, dy, ws, M, C, K, target_blocks)
    assert got == splits, (got, splits)
    dw = torch.empty((K, C), dtype=torch.float32, device=x.device)
    native.C.wgrad_reduce(ws, splits, K, C, C, K * C, dw, C, 1.0, False)
    return dw


def qualifies(m: nn.Conv2d) -> bool:
    """The convs the kernels cover (everything else stays on ``F.conv2d``)."""
    return (tuple(m.kernel_size) == (1, 1) and tuple(m.stride) == (1, 1) and tuple(m.dilation) == (1, 1)
            and m.padding in ((0, 0), 0) and m.groups == 1 and m.bias is None
            and m.in_channels % 8 == 0 and m.out_channels % 8 == 0
            and MIN_CH <= m.in_channels <= MAX_CH and MIN_CH <= m.out_channels <= MAX_CH)


class _PointwiseFn(torch.autograd.Function):
    """``x``: logical NCHW, dense in channels_last, 16-bit; ``weight``: the fp32 ``[K, C, 1, 1]`` master."""

    @staticmethod
    def forward(ctx, x, weight):
        K, C = weight.shape[:2]
        # the 16-bit operand of the kernels, derived from the master here (not an autograd op)
        w16 = weight.detach().reshape(K, C).to(x.dtype)
        y = pwconv_fwd(x.permute(0, 2, 3, 1), w16)  # NHWC view of the channels_last storage: no copy
        ctx.save_for_backward(x, w16)
        return y.permute(0, 3, 1, 2)  # channels_last NCHW view

    @staticmethod
    def backward(ctx, gy):
        x, w16 = ctx.saved_tensors
        K, C = w16.shape
        g = gy.permute(0, 2, 3, 1)
        if g.dtype != x.dtype or not g.is_contiguous():
            g = g.to(x.dtype).contiguous()
        dx = None
        if ctx.needs_input_grad[0]:
            dx = pwconv_dgrad(g, w16).permute(0, 3, 1, 2)  # w16^T made here: once per backward, at most 8 MiB
        dw = None
        if ctx.needs_input_grad[1]:
            dw = pwconv_wgrad(x.permute(0, 2, 3, 1), g).view(K, C, 1, 1)  # fp32 all the way
        return dx, dw


class _PointwiseStatsFn(torch.autograd.Function):
    """:class:`_PointwiseFn` whose forward also returns the BatchNorm statistics slots of ``y`` (not differentiable:
    the BatchNorm behind still differentiates through its statistics as a function of ``y``)."""

    @staticmethod
    def forward(ctx, x, weight):
        K, C = weight.shape[:2]
        w16 = weight.detach().reshape(K, C).to(x.dtype)
        y, slots, _ = pwconv_fwd_stats(x.permute(0, 2, 3, 1), w16)
        ctx.save_for_backward(x, w16)
        ctx.mark_non_differentiable(slots)
        return y.permute(0, 3, 1, 2), slots

    @staticmethod
    def backward(ctx, gy, _gslots):
        return _PointwiseFn.backward(ctx, gy)


class PointwiseConv2d(nn.Conv2d):
    """``nn.Conv2d`` (same constructor, parameters and state-dict keys) that runs a qualifying 1x1 conv on the native
    kernels when its input is a 16-bit, dense ``channels_last`` GPU tensor within the kernels' addressing.  CPU, fp32,
    NCHW inputs and non-qualifying configurations take ``F.conv2d`` exactly as the parent does.

    ``emit_stats`` (set by ``ops.convstats.convert_convstats`` when a ``BNAct2d`` directly follows): in training mode
    the native path also forms the BatchNorm statistics of its output and hands them over as the attribute
    ``ops.bnact.CONV_STATS_ATTR = (slots, version)`` of the tensor object it returns."""

    emit_stats = False

    def forward(self, input: torch.Tensor) -> torch.Tensor:
        if (input.is_cuda and input.dtype in _DTYPES and input.dim() == 4 and qualifies(self)
                and input.is_contiguous(memory_format=torch.channels_last) and input.numel() > 0
                and input.data_ptr() % 16 == 0  # the kernels' 16-byte accesses
                and fits(input.numel() // self.in_channels, self.in_channels, self.out_channels)):
            return self._forward_native(input)
        return super().forward(input)

    def _forward_native(self, input: torch.Tensor) -> torch.Tensor:
        # a forward hook (added after the pairing) may return another tensor: the statistics would be wasted work
        if self.emit_stats and self.training and not self._forward_hooks:
            y, slots = _PointwiseStatsFn.apply(input, self.weight)
            setattr(y, CONV_STATS_ATTR, (slots, y._version))
            return y
        return _PointwiseFn.apply(input, self.weight)


def _as_pointwise(conv: nn.Conv2d) -> PointwiseConv2d:
    # the same module state under the new class: parameters (the same Parameter objects), hooks, training flag
    new = PointwiseConv2d.__new__(PointwiseConv2d)
    new.__dict__ = conv.__dict__.copy()
    for k in ("_parameters", "_buffers", "_modules"):
        new.__dict__[k] = conv.__dict__[k].copy()
    return new


def convert_pointwise(model: nn.Module) -> int:
    """Swap every qualifying ``nn.Conv2d`` below ``model`` for a :class:`PointwiseConv2d` holding the same
    ``Parameter``; returns how many were swapped (0 on a second call).  Call it before the parameters are
    flattened (``optim.flat.FlatParams``)."""
    n = 0
    for parent in list(model.modules()):
        for name, child in list(parent.named_children()):
            if type(child) is nn.Conv2d and qualifies(child):
                setattr(parent, name, _as_pointwise(child))
                n += 1
    return n
