"""Depthwise convolution on the native HIP kernels (``csrc/kernels/dwconv.hip``).

Functional ops (the unit-test surface, tests/test_depthwise_gpu.py) over NHWC 16-bit activations and a taps-major
``[R, S, C]`` 16-bit weight, for ``groups == Cin == Cout == C``, square kernels 3 / 5, stride 1 / 2, dilation 1,
padding ``R // 2`` and ``C % 8 == 0``:

* :func:`dwconv_fwd`    forward
* :func:`dwconv_dgrad`  gradient w.r.t. the input (gather form: every element written once)
* :func:`dwconv_wgrad`  gradient w.r.t. the weight, fp32, deterministic (per-block partial slabs + fixed-order sum)

and the drop-in module for the torch engine:

* :class:`DepthwiseConv2d`  an ``nn.Conv2d`` whose forward runs the kernels when the input is a 16-bit
  ``channels_last`` GPU tensor (the torch engine's training activations under autocast) and ``F.conv2d`` otherwise
* :func:`convert_depthwise` swaps every qualifying ``nn.Conv2d`` of a model in place (``--native-depthwise on``)
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import native

# blocks the weight gradient aims for: a few per CU (256 CUs), so the split-K tail stays short
WGRAD_TARGET_BLOCKS = 2048

_DTYPES = (torch.bfloat16, torch.float16)


def _out_size(n: int, stride: int) -> int:
    return (n - 1) // stride + 1  # pad = R // 2, odd R


def dwconv_fwd(x: torch.Tensor, w: torch.Tensor, stride: int = 1) -> torch.Tensor:
    """``y[N, P, Q, C]`` of ``x[N, H, W, C]`` (NHWC contiguous, 16-bit) and ``w[R, S, C]`` (same dtype)."""
    N, H, W, C = x.shape
    R = w.shape[0]
    y = torch.empty((N, _out_size(H, stride), _out_size(W, stride), C), dtype=x.dtype, device=x.device)
    native.C.dwconv_fwd(x, w, y, N, H, W, C, R, stride)
    return y


def dwconv_dgrad(dy: torch.Tensor, w: torch.Tensor, H: int, W: int, stride: int = 1) -> torch.Tensor:
    """``dx[N, H, W, C]`` of ``dy[N, P, Q, C]`` and ``w[R, S, C]``."""
    N, _, _, C = dy.shape
    R = w.shape[0]
    dx = torch.empty((N, H, W, C), dtype=dy.dtype, device=dy.device)
    native.C.dwconv_dgrad(dy, w, dx, N, H, W, C, R, stride)
    return dx


def dwconv_wgrad_plan(npix: int, C: int, R: int, target_blocks: int = WGRAD_TARGET_BLOCKS):
    """``(splits, pixels per split, channel groups)`` the weight gradient uses for ``npix = N * P * Q`` pixels."""
    return tuple(native.C.dwconv_wgrad_plan(npix, C, R, target_blocks))


def dwconv_wgrad(x: torch.Tensor, dy: torch.Tensor, R: int, stride: int = 1,
                 target_blocks: int = WGRAD_TARGET_BLOCKS) -> torch.Tensor:
    """``dw[R, S, C]`` (fp32) of ``x[N, H, W, C]`` and ``dy[N, P, Q, C]``."""
    N, H, W, C = x.shape
    npix = dy.numel() // C
    splits = dwconv_wgrad_plan(npix, C, R, target_blocks)[0]
    ws = torch.empty((splits, R * R, C), dtype=torch.float32, device=x.device)
    got = native.C.dwconv_wgrad(x, dy, ws, N, H, W, C, R, stride, target_blocks)
    assert got == splits, (got, splits)
    dw = torch.empty((R, R, C), dtype=torch.float32, device=x.device)
    native.C.wgrad_reduce(ws, splits, R * R, C, C, R * R * C, dw, C, 1.0, False)
    return dw


def qualifies(m: nn.Conv2d) -> bool:
    """The convs the kernels cover (everything else stays on ``F.conv2d``)."""
    k = m.kernel_size
    return (m.groups == m.in_channels == m.out_channels and k in ((3, 3), (5, 5))
            and tuple(m.stride) in ((1, 1), (2, 2)) and tuple(m.dilation) == (1, 1)
            and m.padding == (k[0] // 2, k[1] // 2) and m.padding_mode == "zeros" and m.bias is None
            and m.in_channels % 8 == 0)


class _DepthwiseFn(torch.autograd.Function):
    """``x``: logical NCHW, dense in channels_last, 16-bit; ``weight``: the fp32 ``[C, 1, R, S]`` master."""

    @staticmethod
    def forward(ctx, x, weight, stride):
        C, _, R, S = weight.shape
        # the 16-bit taps-major operand of the kernels, derived from the master here (not an autograd op)
        w16 = weight.detach().reshape(C, R * S).t().to(x.dtype).contiguous().view(R, S, C)
        y = dwconv_fwd(x.permute(0, 2, 3, 1), w16, stride)  # NHWC view of the channels_last storage: no copy
        ctx.save_for_backward(x, w16)
        ctx.stride = stride
        return y.permute(0, 3, 1, 2)  # channels_last NCHW view

    @staticmethod
    def backward(ctx, gy):
        x, w16 = ctx.saved_tensors
        R, S, C = w16.shape
        g = gy.permute(0, 2, 3, 1)
        if g.dtype != x.dtype or not g.is_contiguous():
            g = g.to(x.dtype).contiguous()
        xh = x.permute(0, 2, 3, 1)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = dwconv_dgrad(g, w16, xh.shape[1], xh.shape[2], ctx.stride).permute(0, 3, 1, 2)
        dw = None
        if ctx.needs_input_grad[1]:
            # fp32 all the way: [R, S, C] -> the parameter's [C, 1, R, S]
            dw = dwconv_wgrad(xh, g, R, ctx.stride).view(R * S, C).t().reshape(C, 1, R, S)
        return dx, dw, None


class DepthwiseConv2d(nn.Conv2d):
    """``nn.Conv2d`` (same constructor, parameters and state-dict keys) that runs a qualifying depthwise conv on the
    native kernels when its input is a 16-bit, dense ``channels_last`` GPU tensor.  CPU, fp32, NCHW inputs and
    non-qualifying configurations take ``F.conv2d`` exactly as the parent does."""

    def forward(self, input: torch.Tensor) -> torch.Tensor:
        if (input.is_cuda and input.dtype in _DTYPES and input.dim() == 4 and qualifies(self)
                and input.is_contiguous(memory_format=torch.channels_last)):
            return _DepthwiseFn.apply(input, self.weight, self.stride[0])
        return super().forward(input)


def _as_depthwise(conv: nn.Conv2d) -> DepthwiseConv2d:
    # the same module state under the new class: parameters (the same Parameter objects), hooks, training flag
    new = DepthwiseConv2d.__new__(DepthwiseConv2d)
    new.__dict__ = conv.__dict__.copy()
    for k in ("_parameters", "_buffers", "_modules"):
        new.__dict__[k] = conv.__dict__[k].copy()
    return new


def convert_depthwise(model: nn.Module) -> int:
    """Swap every qualifying ``nn.Conv2d`` below ``model`` for a :class:`DepthwiseConv2d` holding the same
    ``Parameter``; returns how many were swapped (0 on a second call).  Call it before the parameters are
    flattened (``optim.flat.FlatParams``)."""
    n = 0
    for parent in list(model.modules()):
        for name, child in list(parent.named_children()):
            if type(child) is nn.Conv2d and qualifies(child):
                setattr(parent, name, _as_depthwise(child))
                n += 1
    return n
