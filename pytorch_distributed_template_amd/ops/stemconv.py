"""The 3x3 / stride 2 / 3-channel first conv of the depthwise-separable models on the native HIP kernels
(``csrc/kernels/stem3x3.hip``).

Functional ops (the unit-test surface, tests/test_stem3x3_gpu.py) over the fp32 NHWC image ``x[N, H, W, 3]`` (the
storage of a dense ``channels_last`` ``[N, 3, H, W]`` tensor), a 16-bit KRSC weight ``w[K, 3, 3, 3]`` and 16-bit NHWC
``y`` / ``dy`` ``[N, P, Q, K]`` (``P = (H - 1) // 2 + 1``, ``Q`` likewise), for kernel 3x3, stride 2, padding 1, dilation
1, groups 1, no bias, ``K % 8 == 0`` and ``8 <= K <= 64``.  The kernels round the image to the 16-bit dtype in registers
(the value ``x.to(dtype)`` has), so the arithmetic is ``F.conv2d``'s under autocast without a 16-bit copy of the image:

* :func:`stem3x3_fwd`    forward
* :func:`stem3x3_wgrad`  gradient w.r.t. the weight, fp32 KRSC, deterministic (per-split partial slabs + fixed-order sum)

There is no gradient w.r.t. the image.  The drop-in module for the torch engine:

* :class:`StemConv2d`   an ``nn.Conv2d`` whose forward runs the kernels when the input is an fp32 ``channels_last`` GPU
  tensor that needs no gradient and CUDA autocast is on (the torch engine's training image) and ``F.conv2d`` otherwise
* :func:`convert_stem`  swaps every qualifying ``nn.Conv2d`` of a model in place (``--native-stem on``)
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import native

# blocks the weight gradient aims for: the 512 that are resident at once (256 CUs, two 64 KiB-LDS blocks on each).
# More splits cost more in wgrad_reduce, whose 864 outputs each sum the splits serially, than they gain in the kernel
# (profiles/stem3x3_mi355x.md)
WGRAD_TARGET_BLOCKS = 512
MIN_K, MAX_K = 8, 64

_DTYPES = (torch.bfloat16, torch.float16)


def out_hw(H: int, W: int):
    return (H - 1) // 2 + 1, (W - 1) // 2 + 1


def fits(N: int, H: int, W: int, K: int) -> bool:
    """The kernels' contract on sizes (output width, pixels one launch addresses, bytes of one image)."""
    return bool(native.C.stem3x3_fits(N, H, W, K))


def stem3x3_fwd(x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """``y[N, P, Q, K]`` (``w``'s dtype) of the fp32 NHWC image ``x[N, H, W, 3]`` and the 16-bit KRSC ``w[K, 3, 3, 3]``."""
    N, H, W, _ = x.shape
    K = w.shape[0]
    P, Q = out_hw(H, W)
    y = torch.empty((N, P, Q, K), dtype=w.dtype, device=x.device)
    native.C.stem3x3_fwd(x, w, y, N, H, W, K)
    return y


def stem3x3_wgrad_plan(M: int, K: int, target_blocks: int = WGRAD_TARGET_BLOCKS):
    """``(splits, pixels per split)`` the weight gradient uses for ``M = N * P * Q`` output pixels."""
    return tuple(native.C.stem3x3_wgrad_plan(M, K, target_blocks))


def stem3x3_wgrad(x: torch.Tensor, dy: torch.Tensor, target_blocks: int = WGRAD_TARGET_BLOCKS) -> torch.Tensor:
    """``dw[K, 3, 3, 3]`` (fp32, KRSC) of the fp32 NHWC image ``x`` and the 16-bit ``dy[N, P, Q, K]``."""
    N, H, W, _ = x.shape
    K = dy.shape[-1]
    splits = stem3x3_wgrad_plan(dy.numel() // K, K, target_blocks)[0]
    ws = torch.empty((splits, K, 32), dtype=torch.float32, device=x.device)
    got = native.C.stem3x3_wgrad(x, dy, ws, N, H, W, K, target_blocks)
    assert got == splits, (got, splits)
    dw = torch.empty((K, 3, 3, 3), dtype=torch.float32, device=x.device)
    native.C.wgrad_reduce(ws, splits, K, 27, 32, K * 32, dw, 27, 1.0, False)
    return dw


def qualifies(m: nn.Conv2d) -> bool:
    """The convs the kernels cover (everything else stays on ``F.conv2d``)."""
    return (m.in_channels == 3 and tuple(m.kernel_size) == (3, 3) and tuple(m.stride) == (2, 2)
            and m.padding in ((1, 1), 1) and tuple(m.dilation) == (1, 1) and m.groups == 1 and m.bias is None
            and m.out_channels % 8 == 0 and MIN_K <= m.out_channels <= MAX_K)


def _autocast_dtype():
    """The CUDA autocast dtype, or None when CUDA autocast is off."""
    if not torch.is_autocast_enabled():
        return None
    get = getattr(torch, "get_autocast_dtype", None)
    return get("cuda") if get is not None else torch.get_autocast_gpu_dtype()


class _StemFn(torch.autograd.Function):
    """``x``: logical NCHW fp32, dense in channels_last, no gradient; ``weight``: the fp32 ``[K, 3, 3, 3]`` (K, C, R, S)
    master; ``dtype``: the compute dtype."""

    @staticmethod
    def forward(ctx, x, weight, dtype):
        # the 16-bit KRSC operand of the kernels, derived from the master here (not an autograd op)
        w16 = weight.detach().permute(0, 2, 3, 1).to(dtype).contiguous()
        y = stem3x3_fwd(x.permute(0, 2, 3, 1), w16)  # NHWC view of the channels_last storage: no copy
        ctx.save_for_backward(x)
        ctx.dtype = dtype
        return y.permute(0, 3, 1, 2)  # channels_last NCHW view

    @staticmethod
    def backward(ctx, gy):
        (x,) = ctx.saved_tensors
        dw = None
        if ctx.needs_input_grad[1]:
            g = gy.permute(0, 2, 3, 1)
            if g.dtype != ctx.dtype or not g.is_contiguous():
                g = g.to(ctx.dtype).contiguous()
            # fp32 all the way; KRSC -> the parameter's (K, C, R, S)
            dw = stem3x3_wgrad(x.permute(0, 2, 3, 1), g).permute(0, 3, 1, 2)
        return None, dw, None


class StemConv2d(nn.Conv2d):
    """``nn.Conv2d`` (same constructor, parameters and state-dict keys) that runs a qualifying first conv on the native
    kernels when its input is an fp32, dense ``channels_last`` GPU image that needs no gradient and CUDA autocast is on
    with a 16-bit dtype.  CPU, no autocast, NCHW or 16-bit inputs, inputs that require grad and non-qualifying
    configurations take ``F.conv2d`` exactly as the parent does."""

    def forward(self, input: torch.Tensor) -> torch.Tensor:
        if (input.is_cuda and input.dtype == torch.float32 and input.dim() == 4 and not input.requires_grad
                and qualifies(self) and input.shape[1] == 3 and input.numel() > 0
                and input.is_contiguous(memory_format=torch.channels_last)):
            dtype = _autocast_dtype()
            if dtype in _DTYPES and fits(input.shape[0], input.shape[2], input.shape[3], self.out_channels):
                return _StemFn.apply(input, self.weight, dtype)
        return super().forward(input)


def _as_stem(conv: nn.Conv2d) -> StemConv2d:
    # the same module state under the new class: parameters (the same Parameter objects), hooks, training flag
    new = StemConv2d.__new__(StemConv2d)
    new.__dict__ = conv.__dict__.copy()
    for k in ("_parameters", "_buffers", "_modules"):
        new.__dict__[k] = conv.__dict__[k].copy()
    return new


def convert_stem(model: nn.Module) -> int:
    """Swap every qualifying ``nn.Conv2d`` below ``model`` for a :class:`StemConv2d` holding the same ``Parameter``;
    returns how many were swapped (0 on a second call).  Call it before the parameters are flattened
    (``optim.flat.FlatParams``)."""
    n = 0
    for parent in list(model.modules()):
        for name, child in list(parent.named_children()):
            if type(child) is nn.Conv2d and qualifies(child):
                setattr(parent, name, _as_stem(child))
                n += 1
    return n
