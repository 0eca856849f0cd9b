"""Global self-attention on the native HIP kernels (``csrc/kernels/mha.hip``): every ViT encoder block.

``y = softmax(scale * q k^T) v`` per (batch, head) over ``1 <= N <= 4096`` tokens and ``heads`` heads of dimension 64: no
bias, no mask, no dropout.  Functional ops (the unit-test surface, tests/test_mha_gpu.py); ``q`` / ``k`` / ``v`` are
16-bit views ``[B, N, heads, 64]`` with any strides that are multiples of 8 (the three slices of the packed in-projection
are such views: no permute copy):

* :func:`mha_attention_fwd`  ``y[B, N, heads * 64]`` (token-major: what ``out_proj`` reads) and the fp32 log-sum-exp of
  every row's scaled scores ``lse[B, heads, N]``, in the base-2 domain (natural log-sum-exp = ``lse * ln 2``)
* :func:`mha_attention_bwd`  ``dq``, ``dk``, ``dv`` (into ``out`` views when given), deterministic: two passes that
  recompute P from ``lse``, no atomics

and the drop-in module for the torch engine:

* :class:`NativeMultiheadAttention`  ``nn.MultiheadAttention`` as ``models.modern.EncoderBlock`` calls it
* :func:`convert_mha`                swaps every qualifying module of a model in place (``--native-mha on``)

The two ``Linear``s stay in torch.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import native
from ._module import DTYPES16, autocast_dtype, swap_children

HEAD_DIM = 64
MAX_TOKENS = 4096


def fits(B: int, heads: int, N: int, head_dim: int) -> bool:
    return bool(native.C.mha_fits(B, heads, N, head_dim))


def mha_attention_fwd(q, k, v, scale: float):
    """``(y[B, N, heads * 64], lse[B, heads, N])`` of the views ``q`` / ``k`` / ``v`` ``[B, N, heads, 64]``."""
    B, N, heads, _ = q.shape
    y = torch.empty((B, N, heads * HEAD_DIM), dtype=q.dtype, device=q.device)
    lse = torch.empty((B, heads, N), dtype=torch.float32, device=q.device)
    native.C.mha_fwd(q, k, v, y, lse, scale)
    return y, lse


def mha_attention_bwd(dy, y, q, k, v, lse, scale: float, out=None):
    """``(dq, dk, dv)`` for ``dy[B, N, heads * 64]`` and the forward's ``y`` and ``lse``; ``out``: three views to write
    them into (the slices of one dense ``dqkv``), else three dense tensors."""
    B, N, heads, _ = q.shape
    dq, dk, dv = out if out is not None else (torch.empty((B, N, heads, HEAD_DIM), dtype=q.dtype, device=q.device)
                                              for _ in range(3))
    delta = torch.empty((B, heads, N), dtype=torch.float32, device=q.device)
    native.C.mha_bwd(dy.view(B, N, heads, HEAD_DIM), y, q, k, v, lse, dq, dk, dv, delta, scale)
    return dq, dk, dv


class _PackedFn(torch.autograd.Function):
    """``qkv``: the dense 16-bit ``[B, N, 3 * heads * 64]`` output of the in-projection; returns ``y``."""

    @staticmethod
    def forward(ctx, qkv, heads, scale):
        B, N, _ = qkv.shape
        q, k, v = qkv.view(B, N, 3, heads, HEAD_DIM).unbind(2)
        y, lse = mha_attention_fwd(q, k, v, scale)
        ctx.save_for_backward(qkv, y, lse)
        ctx.heads, ctx.scale = heads, scale
        return y

    @staticmethod
    def backward(ctx, gy):
        qkv, y, lse = ctx.saved_tensors
        B, N, _ = qkv.shape
        q, k, v = qkv.view(B, N, 3, ctx.heads, HEAD_DIM).unbind(2)
        dqkv = torch.empty_like(qkv)
        if gy.dtype != qkv.dtype or not gy.is_contiguous():
            gy = gy.to(qkv.dtype).contiguous()
        mha_attention_bwd(gy, y, q, k, v, lse, ctx.scale, dqkv.view(B, N, 3, ctx.heads, HEAD_DIM).unbind(2))
        return dqkv, None, None


def qualifies(m: nn.MultiheadAttention) -> bool:
    """The static conditions of the native path: packed self-attention, batch first, head dimension 64."""
    return (m._qkv_same_embed_dim and m.batch_first and m.head_dim == HEAD_DIM and m.bias_k is None
            and m.bias_v is None and not m.add_zero_attn)


class NativeMultiheadAttention(nn.MultiheadAttention):
    """``nn.MultiheadAttention`` (same parameters and state-dict keys) whose attention runs on the native kernels for
    batch-first self-attention without weights, masks or active dropout, on a 3-D GPU input whose in-projection comes
    out 16-bit (16-bit autocast, or a 16-bit module), head dimension 64 and at most 4096 tokens.  Every other call
    takes the parent's forward unchanged."""

    def _native_dtype(self, query, key, value, key_padding_mask, need_weights, attn_mask, is_causal):
        if not (query is key and key is value and query.dim() == 3 and query.is_cuda and not need_weights
                and attn_mask is None and key_padding_mask is None and not is_causal and qualifies(self)
                and not (self.training and self.dropout > 0)
                and fits(query.size(0), self.num_heads, query.size(1), self.head_dim)):
            return None
        dt = autocast_dtype() or (query.dtype if query.dtype == self.in_proj_weight.dtype else None)
        return dt if dt in DTYPES16 else None

    def forward(self, query, key, value, key_padding_mask=None, need_weights=True, attn_mask=None,
                average_attn_weights=True, is_causal=False):
        dt = self._native_dtype(query, key, value, key_padding_mask, need_weights, attn_mask, is_causal)
        if dt is None:
            return super().forward(query, key, value, key_padding_mask=key_padding_mask, need_weights=need_weights,
                                   attn_mask=attn_mask, average_attn_weights=average_attn_weights, is_causal=is_causal)
        qkv = F.linear(query, self.in_proj_weight, self.in_proj_bias).to(dt)
        y = _PackedFn.apply(qkv.contiguous(), self.num_heads, HEAD_DIM ** -0.5)
        return self.out_proj(y), None


def convert_mha(model: nn.Module) -> int:
    """Swap every qualifying ``nn.MultiheadAttention`` below ``model`` for :class:`NativeMultiheadAttention` holding the
    same ``Parameter`` objects; returns how many were swapped (0 on a second call)."""
    return swap_children(model, {nn.MultiheadAttention: NativeMultiheadAttention}, qualifies)
