"""7x7 depthwise convolution on the native HIP kernels (``csrc/kernels/dwconv7.hip``): ConvNeXt's ``CNBlock`` conv.

Functional ops (the unit-test surface, tests/test_dwconv7_gpu.py) over NHWC 16-bit activations, a taps-major
``[7, 7, C]`` 16-bit weight and an optional 16-bit ``[C]`` bias, for ``groups == Cin == Cout == C``, kernel 7x7,
stride 1, padding 3, dilation 1 and ``C % 8 == 0``:

* :func:`dwconv7_fwd`    forward (bias added in fp32 before the one rounding)
* :func:`dwconv7_dgrad`  gradient w.r.t. the input (the same kernel over ``dy`` with the taps flipped)
* :func:`dwconv7_wgrad`  gradients w.r.t. the weight and the bias, fp32, deterministic (per-block partial slabs +
  fixed-order sum)

and the drop-in module for the torch engine:

* :class:`DepthwiseConv7x7`  an ``nn.Conv2d`` whose forward runs the kernels when the input is a dense
  ``channels_last`` GPU tensor that is 16-bit, or fp32 under 16-bit CUDA autocast (ConvNeXt's residual stream), and
  ``F.conv2d`` otherwise
* :func:`convert_depthwise7` swaps every qualifying ``nn.Conv2d`` of a model in place (``--native-dw7 on``)
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import native
from ._module import DTYPES16, autocast_dtype, grad_nhwc, nchw, nhwc, swap_children

# blocks the weight gradient aims for: a few per CU (256 CUs), so the split tail stays short
WGRAD_TARGET_BLOCKS = 2048


def dwconv7_fwd(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor | None = None) -> torch.Tensor:
    """``y[N, H, W, C]`` of ``x[N, H, W, C]`` (NHWC contiguous, 16-bit), ``w[7, 7, C]`` and ``bias[C]`` (same dtype)."""
    N, H, W, C = x.shape
    y = torch.empty_like(x)
    native.C.dwconv7_fwd(x, w, bias, y, N, H, W, C)
    return y


def dwconv7_dgrad(dy: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """``dx[N, H, W, C]`` of ``dy[N, H, W, C]`` and ``w[7, 7, C]``."""
    N, H, W, C = dy.shape
    dx = torch.empty_like(dy)
    native.C.dwconv7_dgrad(dy, w, dx, N, H, W, C)
    return dx


def dwconv7_wgrad_plan(npix: int, C: int, target_blocks: int = WGRAD_TARGET_BLOCKS):
    """``(splits, pixels per split, channel groups)`` the weight gradient uses for ``npix = N * H * W`` pixels."""
    return tuple(native.C.dwconv7_wgrad_plan(npix, C, target_blocks))


def dwconv7_wgrad(x: torch.Tensor, dy: torch.Tensor, want_bias: bool = True,
                  target_blocks: int = WGRAD_TARGET_BLOCKS):
    """``(dw[7, 7, C], db[C] or None)``, both fp32, of ``x[N, H, W, C]`` and ``dy[N, H, W, C]``."""
    N, H, W, C = x.shape
    splits = dwconv7_wgrad_plan(N * H * W, C, target_blocks)[0]
    ws = torch.empty((splits, 50, C), dtype=torch.float32, device=x.device)
    got = native.C.dwconv7_wgrad(x, dy, ws, N, H, W, C, target_blocks)
    assert got == splits, (got, splits)
    out = torch.empty((50, C), dtype=torch.float32, device=x.device)  # rows 0..48: the taps; row 49: sum of dy
    native.C.wgrad_reduce(ws, splits, 50, C, C, 50 * C, out, C, 1.0, False)
    return out[:49].view(7, 7, C), (out[49] if want_bias else None)


def qualifies7(m: nn.Conv2d) -> bool:
    """The convs the kernels cover (everything else stays on ``F.conv2d``); a bias may be present or not."""
    return (m.groups == m.in_channels == m.out_channels and tuple(m.kernel_size) == (7, 7)
            and tuple(m.stride) == (1, 1) and tuple(m.dilation) == (1, 1) and m.padding == (3, 3)
            and m.padding_mode == "zeros" and m.in_channels % 8 == 0)


class _Depthwise7Fn(torch.autograd.Function):
    """``x``: logical NCHW, dense in channels_last, 16-bit; ``weight`` / ``bias``: the fp32 ``[C, 1, 7, 7]`` / ``[C]``
    masters (``bias`` may be None)."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        C = weight.shape[0]
        # the 16-bit operands of the kernels, derived from the masters here (not autograd ops)
        w16 = weight.detach().reshape(C, 49).t().to(x.dtype).contiguous().view(7, 7, C)
        b16 = None if bias is None else bias.detach().to(x.dtype).contiguous()
        y = dwconv7_fwd(nhwc(x), w16, b16)
        ctx.save_for_backward(x, w16)
        ctx.has_bias = bias is not None
        return nchw(y)

    @staticmethod
    def backward(ctx, gy):
        x, w16 = ctx.saved_tensors
        C = w16.shape[2]
        g = grad_nhwc(gy, x.dtype)
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = nchw(dwconv7_dgrad(g, w16))
        want_b = ctx.has_bias and ctx.needs_input_grad[2]
        if ctx.needs_input_grad[1] or want_b:
            dw, db = dwconv7_wgrad(nhwc(x), g, want_b)
            # fp32 all the way: [7, 7, C] -> the parameter's [C, 1, 7, 7]
            dw = dw.reshape(49, C).t().reshape(C, 1, 7, 7) if ctx.needs_input_grad[1] else None
        return dx, dw, db


class DepthwiseConv7x7(nn.Conv2d):
    """``nn.Conv2d`` (same constructor, parameters and state-dict keys) that runs a qualifying 7x7 depthwise conv on
    the native kernels when its input is a 4-D dense ``channels_last`` GPU tensor that is 16-bit, or fp32 while CUDA
    autocast is on with a 16-bit dtype (then cast by ``input.to(dtype)``, exactly what autocast does in front of
    ``F.conv2d``; the cast is autograd-tracked, so ``dx`` comes back fp32).  CPU, fp32 without autocast, NCHW inputs
    and non-qualifying configurations take ``F.conv2d`` exactly as the parent does."""

    def forward(self, input: torch.Tensor) -> torch.Tensor:
        if (input.is_cuda and input.dim() == 4 and qualifies7(self)
                and input.is_contiguous(memory_format=torch.channels_last)):
            if input.dtype in DTYPES16:
                return _Depthwise7Fn.apply(input, self.weight, self.bias)
            if input.dtype == torch.float32:
                dt = autocast_dtype()
                if dt in DTYPES16:
                    return _Depthwise7Fn.apply(input.to(dt), self.weight, self.bias)
        return super().forward(input)


def convert_depthwise7(model: nn.Module) -> int:
    """Swap every qualifying ``nn.Conv2d`` below ``model`` for a :class:`DepthwiseConv7x7` holding the same
    ``Parameter`` objects; returns how many were swapped (0 on a second call).  Call it before the parameters are
    flattened (``optim.flat.FlatParams``)."""
    return swap_children(model, {nn.Conv2d: DepthwiseConv7x7}, qualifies7)
