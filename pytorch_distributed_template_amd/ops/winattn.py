"""Window attention on the native HIP kernels (``csrc/kernels/winattn.hip``): every Swin, Swin V2 and MaxViT block.

``y = softmax(scale * q k^T + bias [+ -100 where the region labels of query and key differ]) v`` over ``Bw`` windows of
``N <= 64`` tokens and ``heads`` heads of dimension 32.  Functional ops (the unit-test surface,
tests/test_winattn_gpu.py); ``q`` / ``k`` / ``v`` are 16-bit views ``[Bw, N, heads, 32]`` with any strides that are
multiples of 8 (the three slices of the packed qkv ``Linear`` output are such views: no permute copy), ``bias`` is fp32
``[heads, N, N]``, ``region`` is None or uint8 ``[nwin, N]`` (window ``w`` reads row ``w % nwin``):

* :func:`window_attention_plan`  ``(blocks, slabs)``: persistent blocks, dbias partial slabs
* :func:`window_attention_fwd`   ``y[Bw, N, heads * 32]`` (token-major: what the projection reads) and the fp32 row
  statistics ``stat[Bw, heads, N, 2]`` (max, sum)
* :func:`window_attention_bwd`   ``dq``, ``dk``, ``dv`` (into ``out`` views when given) and the fp32 ``dbias``,
  deterministic (per-wave slabs + fixed-order sums)

and the drop-in modules for the torch engine:

* :class:`NativeShiftedWindowAttention`  ``models.modern.ShiftedWindowAttention`` (Swin V1 packed, V2 separate q / k)
* :class:`NativeRelPosAttention`         ``models.modern.RelativePositionalMultiHeadAttention`` (MaxViT)
* :func:`convert_window_attention`       swaps every qualifying module of a model in place (``--native-winattn on``)

Everything around the attention (pad, roll, partition, the ``Linear``s, V2's normalise and logit scale, the bias gather
/ ``cpb_mlp``) stays in torch; ``dbias`` flows back through it by ordinary autograd.
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import native
from ._module import DTYPES16, autocast_dtype, swap_children
from ..models.modern import RelativePositionalMultiHeadAttention, ShiftedWindowAttention

# persistent blocks the kernels are given at most: two per CU (256 CUs)
MAX_BLOCKS = 512
HEAD_DIM = 32
MAX_TOKENS = 64


def window_attention_plan(Bw: int, heads: int, N: int, max_blocks: int | None = None):
    """``(blocks, slabs)`` the kernels use; ``blocks * 4 == slabs * heads``."""
    return tuple(native.C.winattn_plan(Bw, heads, N, max_blocks or MAX_BLOCKS))


def window_attention_fwd(q, k, v, bias, region, scale: float, max_blocks: int | None = None):
    """``(y[Bw, N, heads * 32], stat[Bw, heads, N, 2])`` of the views ``q`` / ``k`` / ``v`` ``[Bw, N, heads, 32]``."""
    Bw, N, heads, _ = q.shape
    y = torch.empty((Bw, N, heads * HEAD_DIM), dtype=q.dtype, device=q.device)
    stat = torch.empty((Bw, heads, N, 2), dtype=torch.float32, device=q.device)
    native.C.winattn_fwd(q, k, v, bias, region, y, stat, scale, max_blocks or MAX_BLOCKS)
    return y, stat


def window_attention_bwd(dy, q, k, v, bias, region, stat, scale: float, out=None, max_blocks: int | None = None):
    """``(dq, dk, dv, dbias[heads, N, N])`` for ``dy[Bw, N, heads * 32]``; ``out``: three views to write dq / dk / dv
    into (the slices of one dense ``dqkv``), else three dense tensors."""
    Bw, N, heads, _ = q.shape
    mb = max_blocks or MAX_BLOCKS
    dq, dk, dv = out if out is not None else (torch.empty((Bw, N, heads, HEAD_DIM), dtype=q.dtype, device=q.device)
                                              for _ in range(3))
    slabs = window_attention_plan(Bw, heads, N, mb)[1]
    cols = heads * N * N
    pad = (slabs + 31) // 32 * 32 if slabs > 64 else slabs  # above 64: 32 neighbours each, then the slabs / 32 sums
    ws = torch.empty((pad, cols), dtype=torch.float32, device=q.device)
    if pad > slabs:
        ws[slabs:].zero_()
    got = native.C.winattn_bwd(dy.view(Bw, N, heads, HEAD_DIM), q, k, v, bias, region, stat, dq, dk, dv, ws, scale, mb)
    assert got == slabs, (got, slabs)
    dbias = torch.empty((heads, N, N), dtype=torch.float32, device=q.device)
    if pad > 64:
        mid = torch.empty((pad // 32, cols), dtype=torch.float32, device=q.device)
        native.C.wgrad_reduce(ws, 32, pad // 32, cols, 32 * cols, cols, mid, cols, 1.0, False)
        ws, pad = mid, pad // 32
    native.C.wgrad_reduce(ws, pad, 1, cols, cols, cols, dbias, cols, 1.0, False)
    return dq, dk, dv, dbias


def fits(Bw: int, heads: int, N: int, head_dim: int) -> bool:
    return bool(native.C.winattn_fits(Bw, heads, N, head_dim))


def _grad16(gy: torch.Tensor, like: torch.Tensor) -> torch.Tensor:
    return gy if gy.dtype == like.dtype and gy.is_contiguous() else gy.to(like.dtype).contiguous()


class _PackedFn(torch.autograd.Function):
    """``qkv``: the dense 16-bit ``[Bw, N, 3 * heads * 32]`` output of the qkv ``Linear``; returns ``y``."""

    @staticmethod
    def forward(ctx, qkv, bias, region, heads, scale):
        Bw, N, _ = qkv.shape
        q, k, v = qkv.view(Bw, N, 3, heads, HEAD_DIM).unbind(2)
        bias = bias.detach()
        y, stat = window_attention_fwd(q, k, v, bias, region, scale)
        ctx.save_for_backward(qkv, bias, stat)
        ctx.region, ctx.heads, ctx.scale = region, heads, scale
        return y

    @staticmethod
    def backward(ctx, gy):
        qkv, bias, stat = ctx.saved_tensors
        Bw, N, _ = qkv.shape
        q, k, v = qkv.view(Bw, N, 3, ctx.heads, HEAD_DIM).unbind(2)
        dqkv = torch.empty_like(qkv)
        out = dqkv.view(Bw, N, 3, ctx.heads, HEAD_DIM).unbind(2)
        dbias = window_attention_bwd(_grad16(gy, qkv), q, k, v, bias, ctx.region, stat, ctx.scale, out)[3]
        return dqkv, dbias if ctx.needs_input_grad[1] else None, None, None, None


class _SeparateFn(torch.autograd.Function):
    """``q`` / ``k`` / ``v``: 16-bit views ``[Bw, N, heads, 32]``; returns ``y``."""

    @staticmethod
    def forward(ctx, q, k, v, bias, region, scale):
        bias = bias.detach()
        y, stat = window_attention_fwd(q, k, v, bias, region, scale)
        ctx.save_for_backward(q, k, v, bias, stat)
        ctx.region, ctx.scale = region, scale
        return y

    @staticmethod
    def backward(ctx, gy):
        q, k, v, bias, stat = ctx.saved_tensors
        dq, dk, dv, dbias = window_attention_bwd(_grad16(gy, q), q, k, v, bias, ctx.region, stat, ctx.scale)
        return dq, dk, dv, dbias if ctx.needs_input_grad[3] else None, None, None


def _native_dtype(x: torch.Tensor, heads: int, head_dim: int, N: int, windows: int, dropout: bool):
    """The 16-bit dtype the qkv ``Linear`` will produce when the module takes the kernels, else None."""
    if not x.is_cuda or dropout or head_dim != HEAD_DIM or N > MAX_TOKENS or not fits(windows, heads, N, head_dim):
        return None
    dt = autocast_dtype() or x.dtype
    return dt if dt in DTYPES16 else None


def region_labels(pH: int, pW: int, ws: int, sh: int, sw: int, device) -> torch.Tensor:
    """uint8 ``[nwin, ws * ws]``: the nine shift regions of the rolled ``pH x pW`` map, per window and token."""
    region = torch.zeros((pH, pW), dtype=torch.uint8)
    cnt = 0
    for hs in ((0, -ws), (-ws, -sh), (-sh, None)):
        for wsl in ((0, -ws), (-ws, -sw), (-sw, None)):
            region[hs[0]:hs[1], wsl[0]:wsl[1]] = cnt
            cnt += 1
    nwin = (pH // ws) * (pW // ws)
    return region.view(pH // ws, ws, pW // ws, ws).permute(0, 2, 1, 3).reshape(nwin, ws * ws).contiguous().to(device)


class NativeShiftedWindowAttention(ShiftedWindowAttention):
    """``ShiftedWindowAttention`` (same parameters, buffers and state-dict keys) whose attention runs on the native
    kernels for a GPU input whose qkv is 16-bit (16-bit autocast, or a 16-bit module), head dimension 32, window
    tokens <= 64 and no active attention dropout.  The bias stays fp32 and is not repeated per window; the shift mask
    is a cached uint8 label table.  Every other input takes the parent's forward unchanged."""

    def _region(self, pH, pW, ws, sh, sw, device):
        cache = self.__dict__.setdefault("_region_cache", {})
        key = (pH, pW, sh, sw, str(device))
        if key not in cache:
            cache[key] = region_labels(pH, pW, ws, sh, sw, device)
        return cache[key]

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        B, H, W, C = x.shape
        ws = self.window_size[0]
        pH, pW = H + (ws - H % ws) % ws, W + (ws - W % ws) % ws
        nwin = (pH // ws) * (pW // ws)
        heads = self.num_heads
        dt = _native_dtype(x, heads, C // heads, ws * ws, B * nwin, self.training and self.attention_dropout > 0)
        if dt is None:
            return super().forward(x)
        x = F.pad(x, (0, 0, 0, pW - W, 0, pH - H))
        sh = self.shift_size[0] if ws < pH else 0
        sw = self.shift_size[1] if ws < pW else 0
        if sh or sw:
            x = torch.roll(x, shifts=(-sh, -sw), dims=(1, 2))
        x = x.view(B, pH // ws, ws, pW // ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(B * nwin, ws * ws, C)
        qkv_bias = self.qkv.bias
        if self.v2:  # the key bias is held at zero
            qkv_bias = torch.cat([qkv_bias[:C], torch.zeros_like(qkv_bias[C:2 * C]), qkv_bias[2 * C:]])
        qkv = F.linear(x, self.qkv.weight, qkv_bias).to(dt)
        bias = self._bias()[0].float().contiguous()  # [heads, N, N]: fp32, differentiable
        region = self._region(pH, pW, ws, sh, sw, x.device) if sh or sw else None
        if self.v2:
            q, k, v = qkv.view(x.size(0), x.size(1), 3, heads, HEAD_DIM).unbind(2)
            scale = torch.clamp(self.logit_scale, max=math.log(100.0)).exp().view(1, 1, heads, 1)
            q = (F.normalize(q, dim=-1) * scale).to(dt)
            k = F.normalize(k, dim=-1).to(dt)
            y = _SeparateFn.apply(q.contiguous(), k.contiguous(), v, bias, region, 1.0)
        else:
            y = _PackedFn.apply(qkv.contiguous(), bias, region, heads, HEAD_DIM ** -0.5)
        y = self.proj(y)
        y = F.dropout(y, self.dropout, self.training)
        y = y.view(B, pH // ws, pW // ws, ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(B, pH, pW, C)
        if sh or sw:
            y = torch.roll(y, shifts=(sh, sw), dims=(1, 2))
        return y[:, :H, :W, :].contiguous()


class NativeRelPosAttention(RelativePositionalMultiHeadAttention):
    """``RelativePositionalMultiHeadAttention`` (MaxViT) with the native path of
    :class:`NativeShiftedWindowAttention`: the packed qkv, the fp32 bias, no region."""

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        B, G, P, D = x.shape
        dt = _native_dtype(x, self.n_heads, self.head_dim, P, B * G, False)
        if dt is None:
            return super().forward(x)
        qkv = self.to_qkv(x).to(dt).reshape(B * G, P, 3 * self.n_heads * HEAD_DIM)
        bias = self.get_relative_positional_bias()[0].float().contiguous()
        y = _PackedFn.apply(qkv.contiguous(), bias, None, self.n_heads, self.scale_factor)
        return self.merge(y).view(B, G, P, D)


def qualifies(m: nn.Module) -> bool:
    """The attention modules the kernels cover: head dimension 32 and at most 64 tokens per window."""
    if isinstance(m, ShiftedWindowAttention):
        return m.qkv.in_features // m.num_heads == HEAD_DIM and m.window_size[0] * m.window_size[1] <= MAX_TOKENS
    return m.head_dim == HEAD_DIM and m.max_seq_len <= MAX_TOKENS


def convert_window_attention(model: nn.Module) -> int:
    """Swap every qualifying ``ShiftedWindowAttention`` / ``RelativePositionalMultiHeadAttention`` below ``model`` for
    its native subclass holding the same ``Parameter`` objects; returns how many were swapped (0 on a second call)."""
    return swap_children(model, {ShiftedWindowAttention: NativeShiftedWindowAttention,
                                 RelativePositionalMultiHeadAttention: NativeRelPosAttention}, qualifies)
