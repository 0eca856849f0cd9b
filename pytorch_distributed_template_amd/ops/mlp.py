"""The channel MLP ``Linear(C, Hd) -> GELU -> Linear(Hd, Co)`` of ConvNeXt, Swin and MaxViT blocks on the native HIP
kernels (``csrc/kernels/mlp.hip`` around the hidden tensor, ``csrc/kernels/pwconv.hip`` for the first Linear).

Functional ops (the unit-test surface, tests/test_mlp_gpu.py) over dense 16-bit ``[M, channels]`` tensors, a 16-bit
``w2[Co, Hd]`` and the fp32 biases ``b1[Hd]``, ``b2[Co]``; ``C``, ``Hd``, ``Co`` multiples of 8, ``8 <= C, Co <= 512``,
``8 <= Hd <= 2048``:

* :func:`mlp_fits`            the kernels' contract on sizes
* :func:`mlp_fc2_fwd`         ``y = round16(gelu(z0 + b1) @ w2.T + b2)`` from ``z0 = round16(x @ w1.T)``
* :func:`mlp_fc2_dgrad`       ``dz = round16((dy @ w2) * gelu'(z0 + b1))`` and the fp32 ``db1 = colsum(dz)`` in one kernel
* :func:`mlp_fc2_wgrad_plan`  ``(splits, rows per split, Hd tiles, Co tiles, chain)`` of the weight gradient
* :func:`mlp_fc2_wgrad`       ``dw2 = dy.T @ round16(gelu(z0 + b1))``, fp32, deterministic

and the conversion for the torch engine:

* :func:`convert_mlp`  re-classes every ``nn.Sequential`` (or ``models.modern._MLPBlock``) that holds such a run of
  modules so that its forward runs the run on the kernels under 16-bit CUDA autocast (``--native-mlp on``)

The hidden tensor is written once and read once in the forward (``z0``; ``h = gelu(z0 + b1)`` exists only in LDS) and
moves five times in the backward, where the stock ops move it four and eight times, and only ``z0`` is kept for the
backward instead of ``z0`` and ``h``.  The bias ``b1`` enters in fp32 AFTER ``z0 = x @ w1.T`` was rounded to 16 bits;
stock autocast rounds ``x @ w1.T + b1`` once.  GELU, its derivative and both biases are fp32 from the fp32 parameters.
A converted model is therefore not bit-identical to the stock one.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import native
from ._module import DTYPES16, autocast_dtype, reclass
from .pointwise import pwconv_dgrad, pwconv_fwd, pwconv_wgrad
from ..models.modern import _MLPBlock

# blocks the weight gradient aims for: a few per CU (256 CUs, two 64 KiB-LDS blocks resident on each)
WGRAD_TARGET_BLOCKS = 1024


def mlp_fits(M: int, C: int, Hd: int, Co: int) -> bool:
    """The kernels' contract on sizes (``M`` rows, widths ``C -> Hd -> Co``)."""
    return bool(native.C.mlp_fits(M, C, Hd, Co))


def mlp_fc2_fwd(z0: torch.Tensor, b1: torch.Tensor, w2: torch.Tensor, b2: torch.Tensor) -> torch.Tensor:
    """``y[..., Co]`` of ``z0[..., Hd]`` (dense, 16-bit), ``w2[Co, Hd]`` (same dtype) and the fp32 ``b1``, ``b2``."""
    Co, Hd = w2.shape
    y = torch.empty(z0.shape[:-1] + (Co,), dtype=z0.dtype, device=z0.device)
    native.C.mlp_fc2_fwd(z0, b1, w2, b2, y, z0.numel() // Hd, Hd, Co)
    return y


def mlp_fc2_dgrad(dy: torch.Tensor, w2: torch.Tensor, z0: torch.Tensor, b1: torch.Tensor, max_blocks: int = 0):
    """``(dz[..., Hd], db1[Hd] fp32, (partial_rows, chain))``; ``w2[Co, Hd]`` is transposed once here.  ``max_blocks``:
    persistent blocks the launch aims for (0: the default); ``chain`` is the longest run of fp32 additions an element of
    ``db1`` passes through."""
    Co, Hd = w2.shape
    dz = torch.empty_like(z0)
    db1 = torch.empty(Hd, dtype=torch.float32, device=z0.device)
    rows, chain = native.C.mlp_fc2_dgrad(dy, w2.t().contiguous(), z0, b1, dz, db1, z0.numel() // Hd, Hd, Co, max_blocks)
    return dz, db1, (rows, chain)


def mlp_fc2_wgrad_plan(M: int, Hd: int, Co: int, target_blocks: int = WGRAD_TARGET_BLOCKS):
    """``(splits, rows per split, Hd tiles, Co tiles, chain)`` the weight gradient uses for ``M`` rows; ``chain``: the
    roundings of ``2**-24`` an element may pass through, the fold of the slabs included."""
    return tuple(native.C.mlp_fc2_wgrad_plan(M, Hd, Co, target_blocks))


def mlp_fc2_wgrad(z0: torch.Tensor, b1: torch.Tensor, dy: torch.Tensor,
                  target_blocks: int = WGRAD_TARGET_BLOCKS) -> torch.Tensor:
    """``dw2[Co, Hd]`` (fp32) of ``z0[..., Hd]``, ``b1`` and ``dy[..., Co]``."""
    Hd, Co = z0.shape[-1], dy.shape[-1]
    M = z0.numel() // Hd
    splits = mlp_fc2_wgrad_plan(M, Hd, Co, target_blocks)[0]
    ws = torch.empty((splits, Co, Hd), dtype=torch.float32, device=z0.device)
    got = native.C.mlp_fc2_wgrad(z0, b1, dy, ws, M, Hd, Co, target_blocks)
    assert got == splits, (got, splits)
    dw = torch.empty((Co, Hd), dtype=torch.float32, device=z0.device)
    native.C.wgrad_reduce(ws, splits, Co, Hd, Hd, Co * Hd, dw, Hd, 1.0, False)
    return dw


class _MLPFn(torch.autograd.Function):
    """``x``: dense ``[..., C]``, 16-bit or fp32 (cast once, as autocast's Linear would); ``w1`` .. ``b2``: the fp32
    parameters of the two Linears; ``dtype``: the 16-bit dtype of the kernels."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, dtype):
        C = x.shape[-1]
        x16 = x.detach().reshape(-1, C).to(dtype)
        # the 16-bit operands of the kernels, derived from the masters here (not autograd ops)
        w1h, w2h = w1.detach().to(dtype), w2.detach().to(dtype)
        z0 = pwconv_fwd(x16, w1h)
        y = mlp_fc2_fwd(z0, b1.detach(), w2h, b2.detach())
        ctx.save_for_backward(x16, w1h, w2h, z0, b1)
        ctx.xmeta = (x.shape, x.dtype)
        return y.view(x.shape[:-1] + (w2.shape[0],))

    @staticmethod
    def backward(ctx, gy):
        x16, w1h, w2h, z0, b1 = ctx.saved_tensors
        shape, xdtype = ctx.xmeta
        need = ctx.needs_input_grad
        b1 = b1.detach()
        g = gy.reshape(-1, w2h.shape[0])
        if g.dtype != x16.dtype or not g.is_contiguous():
            g = g.to(x16.dtype).contiguous()
        dx = dw1 = db1 = dw2 = db2 = None
        if need[4]:
            db2 = torch.empty(g.shape[1], dtype=torch.float32, device=g.device)
            native.C.colsum(g, g.shape[0], g.shape[1], g.shape[1], db2, 1.0)
        if need[3]:
            dw2 = mlp_fc2_wgrad(z0, b1, g)
        if need[0] or need[1] or need[2]:
            dz, db1, _ = mlp_fc2_dgrad(g, w2h, z0, b1)
            if need[1]:
                dw1 = pwconv_wgrad(x16, dz)
            if need[0]:
                dx = pwconv_dgrad(dz, w1h).view(shape).to(xdtype)  # w1h^T made there: once per backward
        return dx, dw1, db1 if need[2] else None, dw2, db2, None


def _run_at(mods, i: int, x: torch.Tensor | None = None):
    """``(fc1, fc2, slots)`` when the modules from slot ``i`` on form a run -- a biased ``nn.Linear``, an exact-erf
    ``nn.GELU``, optionally an ``nn.Dropout``, a biased ``nn.Linear`` of matching width, the widths inside the
    contract, no forward (pre-)hook on any of them (the fused path does not call them) -- else None.  With ``x`` (the
    tensor about to enter slot ``i``) the run-time conditions are decided here as well: a dense GPU tensor under 16-bit
    CUDA autocast, 16-bit or fp32, the dropout inactive, fp32 parameters on its device, the row count inside the
    contract."""
    if i + 2 >= len(mods):
        return None
    run = [mods[i], mods[i + 1], mods[i + 2]]
    if type(run[2]) is nn.Dropout and i + 3 < len(mods):
        run.append(mods[i + 3])
    fc1, act, fc2 = run[0], run[1], run[-1]
    if not (type(fc1) is nn.Linear and type(fc2) is nn.Linear and type(act) is nn.GELU and act.approximate == "none"
            and fc1.bias is not None and fc2.bias is not None and fc2.in_features == fc1.out_features
            and mlp_fits(1, fc1.in_features, fc1.out_features, fc2.out_features)
            and not any(m._forward_hooks or m._forward_pre_hooks for m in run)):
        return None
    if x is not None:
        drop = run[2] if len(run) == 4 else None
        dt = autocast_dtype()
        params = (fc1.weight, fc1.bias, fc2.weight, fc2.bias)
        if not (x.is_cuda and dt in DTYPES16 and x.dtype in (dt, torch.float32) and x.dim() >= 1
                and x.shape[-1] == fc1.in_features and x.numel() > 0 and x.is_contiguous() and x.data_ptr() % 16 == 0
                and (drop is None or drop.p == 0 or not drop.training)
                and all(p.dtype == torch.float32 and p.device == x.device and p.is_contiguous() for p in params)
                and mlp_fits(x.numel() // fc1.in_features, fc1.in_features, fc1.out_features, fc2.out_features)):
            return None
    return fc1, fc2, len(run)


def _forward(self, input):
    """``nn.Sequential.forward`` that runs every run of :func:`_run_at` through :class:`_MLPFn` and calls every other
    child as the stock forward does."""
    mods = list(self._modules.values())
    i = 0
    while i < len(mods):
        run = _run_at(mods, i, input) if torch.is_tensor(input) else None
        if run is None:
            input = mods[i](input)
            i += 1
        else:
            fc1, fc2, n = run
            input = _MLPFn.apply(input, fc1.weight, fc1.bias, fc2.weight, fc2.bias, autocast_dtype())
            i += n
    return input


class NativeMLPSequential(nn.Sequential):
    """``nn.Sequential`` (same children, parameters and state-dict keys) whose forward runs each ``Linear -> GELU ->
    [Dropout] -> Linear`` run of its slots on the native kernels when the tensor reaching the run is a dense GPU tensor
    under 16-bit CUDA autocast and the dropout is inactive; everywhere else (CPU, no autocast, active dropout, outside the
    contract) it calls the children exactly as ``nn.Sequential.forward`` does."""
    forward = _forward


class NativeMLPBlock(_MLPBlock):
    """``models.modern._MLPBlock`` (Swin's and ViT's MLP) with the forward of :class:`NativeMLPSequential`."""
    forward = _forward


KINDS = {nn.Sequential: NativeMLPSequential, _MLPBlock: NativeMLPBlock}


def _runs(m: nn.Module) -> int:
    mods, i, n = list(m._modules.values()), 0, 0
    while i < len(mods):
        run = _run_at(mods, i)
        i += run[2] if run else 1
        n += run is not None
    return n


def convert_mlp(model: nn.Module) -> int:
    """Re-class every ``nn.Sequential`` / ``_MLPBlock`` below ``model`` that holds a run (:func:`_run_at`) to its native
    subclass holding the same children; returns the number of runs converted (0 on a second call: subclasses are not
    looked at).  Call it before the parameters are flattened (``optim.flat.FlatParams``)."""
    n = 0
    for parent in list(model.modules()):
        for name, child in list(parent.named_children()):
            if type(child) in KINDS and type(child).forward is nn.Sequential.forward:
                k = _runs(child)
                if k:
                    setattr(parent, name, reclass(child, KINDS[type(child)]))
                    n += k
    return n
