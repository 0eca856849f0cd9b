"""LayerNorm on the native HIP kernels (``csrc/kernels/layernorm.hip``): every ConvNeXt, ViT, Swin and MaxViT block.

Functional ops (the unit-test surface, tests/test_layernorm_gpu.py) over a dense ``[rows, C]`` tensor normalised over
``C`` (``C % 8 == 0``, ``8 <= C <= 2048``), fp32 ``gamma`` / ``beta`` (``beta`` may be None):

* :func:`layernorm_plan`  ``(L, NV, blocks)``: lanes per row, 8-channel vectors per lane, persistent blocks
* :func:`layernorm_fwd`   ``y`` (16-bit), ``mean`` and ``rstd`` (fp32) from a 16-bit or fp32 ``x`` in one pass
* :func:`layernorm_bwd`   ``dx`` (the dtype of ``x``) and the fp32 ``dgamma`` / ``dbeta`` in one pass, deterministic
  (per-block partial rows + fixed-order sums)

and the drop-in modules for the torch engine:

* :class:`NativeLayerNorm`    an ``nn.LayerNorm`` whose forward runs the kernels under 16-bit CUDA autocast
* :class:`NativeLayerNorm2d`  the same for ``models.modern.LayerNorm2d`` (the permuted view of a ``channels_last``
  tensor is the ``[rows, C]`` tensor: no copy)
* :func:`convert_layernorm`   swaps every qualifying LayerNorm of a model in place (``--native-layernorm on``)

The native result has the autocast dtype: it is "fp32 LayerNorm, one rounding", which is what the ``nn.Linear`` or
``nn.Conv2d`` behind it would have made of the stock fp32 result.  A consumer other than a GEMM (Swin V2's post-norm
residual add, for one) sees a 16-bit tensor where stock autocast gives fp32.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import native
from ._module import DTYPES16, autocast_dtype, nchw, nhwc, swap_children
from ..models.modern import LayerNorm2d

# persistent blocks the kernels are given at most: four per CU (256 CUs)
MAX_BLOCKS = 1024


def layernorm_plan(rows: int, C: int, max_blocks: int | None = None):
    """``(L, NV, blocks)`` the kernels use for a ``[rows, C]`` tensor."""
    return tuple(native.C.layernorm_plan(rows, C, max_blocks or MAX_BLOCKS))


def layernorm_fwd(x2d: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor | None, eps: float,
                  out_dtype: torch.dtype, max_blocks: int | None = None):
    """``(y[rows, C] in out_dtype, mean[rows], rstd[rows])`` of ``x2d[rows, C]`` (``out_dtype`` or fp32)."""
    rows, C = x2d.shape
    y = torch.empty((rows, C), dtype=out_dtype, device=x2d.device)
    mean = torch.empty(rows, dtype=torch.float32, device=x2d.device)
    rstd = torch.empty_like(mean)
    native.C.layernorm_fwd(x2d, gamma, beta, y, mean, rstd, rows, C, eps, max_blocks or MAX_BLOCKS)
    return y, mean, rstd


def layernorm_bwd(dy: torch.Tensor, x2d: torch.Tensor, mean: torch.Tensor, rstd: torch.Tensor, gamma: torch.Tensor,
                  want_affine: bool = True, max_blocks: int | None = None):
    """``(dx[rows, C] in x2d's dtype, dgamma[C], dbeta[C])``, the last two fp32, or None without ``want_affine``."""
    rows, C = x2d.shape
    mb = max_blocks or MAX_BLOCKS
    dx = torch.empty_like(x2d)
    if not want_affine:
        native.C.layernorm_bwd(dy, x2d, mean, rstd, gamma, dx, None, rows, C, mb)
        return dx, None, None
    blocks = layernorm_plan(rows, C, mb)[2]
    ws = torch.empty((blocks, 2 * C), dtype=torch.float32, device=x2d.device)
    got = native.C.layernorm_bwd(dy, x2d, mean, rstd, gamma, dx, ws, rows, C, mb)
    assert got == blocks, (got, blocks)
    out = torch.empty((2, C), dtype=torch.float32, device=x2d.device)
    if blocks > 64:  # the plan made it a multiple of 32: 32 neighbours each, then the blocks / 32 sums
        mid = torch.empty((blocks // 32, 2 * C), dtype=torch.float32, device=x2d.device)
        native.C.wgrad_reduce(ws, 32, blocks // 32, 2 * C, 64 * C, 2 * C, mid, 2 * C, 1.0, False)
        ws, blocks = mid, blocks // 32
    native.C.wgrad_reduce(ws, blocks, 1, 2 * C, 2 * C, 2 * C, out, 2 * C, 1.0, False)
    return dx, out[0], out[1]


def fits(C: int) -> bool:
    return C % 8 == 0 and 8 <= C <= 2048


def qualifies(m: nn.LayerNorm) -> bool:
    """The LayerNorms the kernels cover: one normalised dimension inside the contract, with gamma."""
    return len(m.normalized_shape) == 1 and fits(m.normalized_shape[0]) and m.elementwise_affine


def _native_dtype(m: nn.LayerNorm, x: torch.Tensor):
    """The autocast dtype when ``x`` (already ``[..., C]``) takes the kernels, else None."""
    if not (x.is_cuda and qualifies(m) and x.dim() >= 1
            and x.shape[-1] == m.normalized_shape[0] and 0 < x.numel() < 2 ** 40 and x.is_contiguous()
            and x.data_ptr() % 16 == 0 and m.weight.dtype == torch.float32):
        return None
    dt = autocast_dtype()
    return dt if dt in DTYPES16 and x.dtype in (dt, torch.float32) else None


class _LayerNormFn(torch.autograd.Function):
    """``x``: dense ``[..., C]``, 16-bit or fp32, saved as it came; ``weight`` / ``bias``: the fp32 parameters."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps, dtype):
        C = x.shape[-1]
        y, mean, rstd = layernorm_fwd(x.view(-1, C), weight.detach(), None if bias is None else bias.detach(), eps, dtype)
        ctx.save_for_backward(x, weight, mean, rstd)
        ctx.has_bias, ctx.dtype = bias is not None, dtype
        return y.view(x.shape)

    @staticmethod
    def backward(ctx, gy):
        x, weight, mean, rstd = ctx.saved_tensors
        C = x.shape[-1]
        g = gy if gy.dtype == ctx.dtype and gy.is_contiguous() else gy.to(ctx.dtype).contiguous()
        want = ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2])
        dx, dg, db = layernorm_bwd(g.view(-1, C), x.view(-1, C), mean, rstd, weight.detach(), want)
        return (dx.view(x.shape) if ctx.needs_input_grad[0] else None, dg if ctx.needs_input_grad[1] else None,
                db if ctx.has_bias and ctx.needs_input_grad[2] else None, None, None)


class NativeLayerNorm(nn.LayerNorm):
    """``nn.LayerNorm`` (same constructor, parameters and state-dict keys) that runs on the native kernels when its
    input is a dense GPU tensor, 16-bit or fp32, while CUDA autocast is on with a 16-bit dtype, and the module
    normalises one dimension ``C`` (``C % 8 == 0``, ``8 <= C <= 2048``) with ``elementwise_affine=True``.  The result
    then has the autocast dtype (fp32 LayerNorm, rounded once) where ``F.layer_norm`` under autocast returns fp32: the
    ``nn.Linear`` / ``nn.Conv2d`` behind it would round the same values, any other consumer sees 16-bit.  Every other
    input (CPU, no autocast, strided, outside the contract) takes ``F.layer_norm`` exactly as the parent does."""

    def forward(self, input: torch.Tensor) -> torch.Tensor:
        dt = _native_dtype(self, input)
        if dt is not None:
            return _LayerNormFn.apply(input, self.weight, self.bias, self.eps, dt)
        return super().forward(input)


class NativeLayerNorm2d(LayerNorm2d):
    """``models.modern.LayerNorm2d`` with the native path of :class:`NativeLayerNorm` for NCHW inputs that are dense
    in ``channels_last``: their ``permute(0, 2, 3, 1)`` view is the ``[rows, C]`` tensor."""

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if x.dim() == 4:
            xp = nhwc(x)
            dt = _native_dtype(self, xp)
            if dt is not None:
                return nchw(_LayerNormFn.apply(xp, self.weight, self.bias, self.eps, dt))
        return super().forward(x)


def convert_layernorm(model: nn.Module) -> int:
    """Swap every qualifying ``nn.LayerNorm`` / ``LayerNorm2d`` below ``model`` for its native subclass holding the
    same ``Parameter`` objects; returns how many were swapped (0 on a second call).  Call it before the parameters are
    flattened (``optim.flat.FlatParams``)."""
    return swap_children(model, {nn.LayerNorm: NativeLayerNorm, LayerNorm2d: NativeLayerNorm2d}, qualifies)
