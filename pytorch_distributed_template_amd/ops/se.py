"""Squeeze-and-excitation on the native HIP kernels (``csrc/kernels/se.hip``): the SE block of EfficientNet / V2,
MobileNetV3, RegNet-Y and MaxViT's MBConv, ``y = x * gate(fc2(act(fc1(mean_hw(x)))))`` with biased 1x1 ``fc1`` / ``fc2``.

Functional ops (the unit-test surface, tests/test_se_gpu.py) over a dense NHWC 16-bit ``x[N, H, W, C]`` (``C % 8 == 0``,
``8 <= C <= 4096``, squeeze width ``1 <= S <= 512``, ``N * HW * C < 2**40``) and the fp32 master parameters ``w1[S, C]``,
``b1[S]``, ``w2[C, S]``, ``b2[C]``, read as they are; ``act`` is ``"relu"`` or ``"silu"``, ``gate`` ``"sigmoid"`` or
``"hardsigmoid"``:

* :func:`se_plan`  ``(chunks, rows_per_chunk)``: how the two reductions split the HW rows of an image; it fixes their
  summation order
* :func:`se_fwd`   ``y`` (the dtype of ``x``) and the fp32 ``z[N, C]`` (pooled mean), ``u[N, S]`` (``fc1`` output),
  ``s[N, C]`` (gate): two reads of ``x``, one write
* :func:`se_bwd`   ``dx`` and the fp32 ``dw1``, ``db1``, ``dw2``, ``db2``: reads ``dy`` and ``x``, then ``dy`` again, one
  write; no atomics, bit-identical from run to run

and the drop-in modules for the torch engine:

* :class:`NativeSqueezeExcitation`, :class:`NativeRegNetSE`, :class:`NativeSE`  subclasses of the three SE classes of
  ``models/`` whose forward runs the kernels on a 16-bit dense ``channels_last`` GPU input
* :func:`convert_se`  swaps every qualifying module of a model in place (``--native-se on``)

All gate math (``z``, ``u``, ``s``) is fp32 from the fp32 parameters; ``y = round(x * s)`` and ``dx = round(dy * s + g)``
are rounded once.  Stock autocast runs ``fc1`` / ``fc2`` and the gate in the 16-bit dtype, so the native gate is the more
accurate of the two: a converted model is not bit-identical to the stock one.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import native
from ._module import DTYPES16, grad_nhwc, nchw, nhwc, swap_children
from ..models.efficient import SqueezeExcitation
from ..models.modern import _RegNetSE, _SE

# blocks the reductions and the persistent streaming passes are given at most: eight per CU (256 CUs)
MAX_BLOCKS = 2048
ACTS = {nn.ReLU: "relu", nn.SiLU: "silu"}
GATES = {nn.Sigmoid: "sigmoid", nn.Hardsigmoid: "hardsigmoid"}
_ACT_ID = {"relu": 0, "silu": 1}
_GATE_ID = {"sigmoid": 0, "hardsigmoid": 1}


def se_plan(N: int, HW: int, C: int, max_blocks: int | None = None):
    """``(chunks, rows_per_chunk)`` of the reductions over an ``[N, HW, C]`` tensor."""
    return tuple(native.C.se_plan(N, HW, C, max_blocks or MAX_BLOCKS))


def _dims(x, w1):
    N, C = x.shape[0], x.shape[-1]
    return N, x.numel() // (N * C), C, w1.shape[0]


def se_fwd(x, w1, b1, w2, b2, act: str, gate: str, max_blocks: int | None = None):
    """``(y, z[N, C], u[N, S], s[N, C])`` of the dense NHWC ``x``; ``y`` has its dtype and shape."""
    N, HW, C, S = _dims(x, w1)
    mb = max_blocks or MAX_BLOCKS
    f32 = dict(dtype=torch.float32, device=x.device)
    y = torch.empty_like(x)
    z, u, s = torch.empty((N, C), **f32), torch.empty((N, S), **f32), torch.empty((N, C), **f32)
    partial = torch.empty((N, se_plan(N, HW, C, mb)[0], C), **f32)
    native.C.se_fwd(x, w1, b1, w2, b2, y, z, u, s, partial, _ACT_ID[act], _GATE_ID[gate], mb)
    return y, z, u, s


def se_bwd(dy, x, w1, w2, z, u, s, act: str, gate: str, want_dx: bool = True, want_params: bool = True,
           max_blocks: int | None = None):
    """``(dx, dw1, db1, dw2, db2)`` from the forward's ``z``, ``u``, ``s``; ``dx`` is None without ``want_dx`` (the
    streaming pass is skipped), the four fp32 parameter gradients without ``want_params`` (``se_wgrad`` is skipped)."""
    N, HW, C, S = _dims(x, w1)
    mb = max_blocks or MAX_BLOCKS
    f32 = dict(dtype=torch.float32, device=x.device)
    dx = torch.empty_like(x) if want_dx else None
    grads = (torch.empty_like(w1), torch.empty(S, **f32), torch.empty_like(w2), torch.empty(C, **f32)) \
        if want_params else (None,) * 4
    partial = torch.empty((N, se_plan(N, HW, C, mb)[0], C), **f32)
    dv, du, g = torch.empty((N, C), **f32), torch.empty((N, S), **f32), torch.empty((N, C), **f32)
    native.C.se_bwd(dy, x, w1, w2, z, u, s, dx, *grads, partial, dv, du, g, _ACT_ID[act], _GATE_ID[gate], mb)
    return (dx,) + grads


class _SEFn(torch.autograd.Function):
    """``x``: 16-bit NCHW, dense in ``channels_last``; ``w1`` .. ``b2``: the fp32 parameters of ``fc1`` / ``fc2``."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, act, gate):
        y, z, u, s = se_fwd(nhwc(x), w1.detach(), b1.detach(), w2.detach(), b2.detach(), act, gate)
        ctx.save_for_backward(x, w1, b1, w2, b2, z, u, s)
        ctx.act, ctx.gate = act, gate
        return nchw(y)

    @staticmethod
    def backward(ctx, gy):
        x, w1, b1, w2, b2, z, u, s = ctx.saved_tensors
        want_dx, want_params = ctx.needs_input_grad[0], any(ctx.needs_input_grad[1:5])
        dx, dw1, db1, dw2, db2 = se_bwd(grad_nhwc(gy, x.dtype), nhwc(x), w1.detach(), w2.detach(), z, u, s, ctx.act,
                                        ctx.gate, want_dx, want_params)
        need = ctx.needs_input_grad
        return (nchw(dx) if want_dx else None, dw1 if need[1] else None, db1 if need[2] else None,
                dw2 if need[3] else None, db2 if need[4] else None, None, None)


def fits(N: int, HW: int, C: int, S: int) -> bool:
    return bool(native.C.se_fits(N, HW, C, S))


def qualifies(m: nn.Module) -> bool:
    """The static conditions of the native path: ReLU / SiLU squeeze, Sigmoid / Hardsigmoid gate, biased 1x1 ``fc1`` /
    ``fc2`` of agreeing widths inside the contract, a global average pool, and no forward (pre-)hook on any of the five
    children (the native path does not call them, so their hooks would not fire)."""
    kids = [getattr(m, k, None) for k in ("avgpool", "fc1", "fc2", "activation", "scale_activation")]
    if any(k is None for k in kids):
        return False
    pool, fc1, fc2, act, gate = kids
    if type(act) not in ACTS or type(gate) not in GATES or type(fc1) is not nn.Conv2d or type(fc2) is not nn.Conv2d:
        return False
    if type(pool) is not nn.AdaptiveAvgPool2d or pool.output_size not in (1, (1, 1)):
        return False
    for fc in (fc1, fc2):
        if not (fc.kernel_size == (1, 1) and fc.stride == (1, 1) and fc.padding == (0, 0) and fc.dilation == (1, 1)
                and fc.groups == 1 and fc.bias is not None and fc.padding_mode == "zeros"):
            return False
    if any(k._forward_hooks or k._forward_pre_hooks for k in kids):
        return False
    C, S = fc1.in_channels, fc1.out_channels
    return fc2.in_channels == S and fc2.out_channels == C and fits(1, 1, C, S)


def _forward(m, x: torch.Tensor, parent):
    """The native path when ``x`` meets the contract and the parameters are fp32 on its device, else ``parent``."""
    params = (m.fc1.weight, m.fc1.bias, m.fc2.weight, m.fc2.bias)
    if (x.is_cuda and x.dtype in DTYPES16 and x.dim() == 4 and x.numel() > 0 and type(m.activation) in ACTS
            and type(m.scale_activation) in GATES and nhwc(x).is_contiguous() and x.data_ptr() % 16 == 0
            and all(p.dtype == torch.float32 and p.device == x.device for p in params)
            and fits(x.shape[0], x.shape[2] * x.shape[3], x.shape[1], m.fc1.out_channels)):
        return _SEFn.apply(x, *params, ACTS[type(m.activation)], GATES[type(m.scale_activation)])
    return parent(x)


class NativeSqueezeExcitation(SqueezeExcitation):
    """``models.efficient.SqueezeExcitation`` (same parameters and state-dict keys) that runs on the native kernels when
    its input is a 16-bit GPU tensor, dense in ``channels_last``, inside the contract (``C % 8 == 0``, ``8 <= C <=
    4096``, ``S <= 512``) and its parameters are fp32 on the same device.  The gate is then computed in fp32 from the fp32
    parameters, where stock autocast computes it in 16 bits.  Every other input (CPU, fp32, NCHW-contiguous, outside the
    contract) takes the parent's forward unchanged."""

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return _forward(self, x, super().forward)


class NativeRegNetSE(_RegNetSE):
    """``models.modern._RegNetSE`` with the native path of :class:`NativeSqueezeExcitation`."""

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return _forward(self, x, super().forward)


class NativeSE(_SE):
    """``models.modern._SE`` (MaxViT's MBConv) with the native path of :class:`NativeSqueezeExcitation`."""

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return _forward(self, x, super().forward)


KINDS = {SqueezeExcitation: NativeSqueezeExcitation, _RegNetSE: NativeRegNetSE, _SE: NativeSE}


def convert_se(model: nn.Module) -> int:
    """Swap every qualifying squeeze-excitation module below ``model`` for its native subclass holding the same
    ``Parameter`` objects; returns how many were swapped (0 on a second call)."""
    return swap_children(model, KINDS, qualifies)
