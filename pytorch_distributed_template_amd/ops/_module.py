"""What the torch engine's drop-in modules (depthwise, depthwise7, stemconv, pointwise, layernorm, bnact, winattn, mha, se,
mlp) share: the 16-bit dtypes, the autocast query, re-classing a module in place, the model walk, and the NHWC views of their
autograd functions.  Each module's eligibility test and its kernels' launch sequences stay with the module."""
from __future__ import annotations

import torch
import torch.nn as nn

DTYPES16 = (torch.bfloat16, torch.float16)


def autocast_dtype():
    """The CUDA autocast dtype, or None when CUDA autocast is off."""
    if not torch.is_autocast_enabled():
        return None
    get = getattr(torch, "get_autocast_dtype", None)
    return get("cuda") if get is not None else torch.get_autocast_gpu_dtype()


def reclass(module: nn.Module, cls, **attrs):
    """``module``'s state under ``cls`` (a subclass of its class): the same ``Parameter`` and buffer objects, hook dicts
    and training flag, in registries of its own, so that registering on the one does not show on the other.  ``attrs``
    become instance attributes.  ``cls.__init__`` is not run."""
    new = cls.__new__(cls)
    new.__dict__ = module.__dict__.copy()
    for k in ("_parameters", "_buffers", "_modules"):
        new.__dict__[k] = module.__dict__[k].copy()
    new.__dict__.update(attrs)
    return new


def swap_children(model: nn.Module, kinds: dict, qualifies) -> int:
    """Replace every child below ``model`` whose exact type is a key of ``kinds`` and that ``qualifies`` by
    :func:`reclass` to ``kinds[type]``; returns how many were replaced (0 on a second call: subclasses are no keys)."""
    n = 0
    for parent in list(model.modules()):
        for name, child in list(parent.named_children()):
            if type(child) in kinds and qualifies(child):
                setattr(parent, name, reclass(child, kinds[type(child)]))
                n += 1
    return n


def nhwc(t: torch.Tensor) -> torch.Tensor:
    """The NHWC view of a logical NCHW tensor: of dense ``channels_last`` storage it is contiguous, no copy."""
    return t.permute(0, 2, 3, 1)


def nchw(t: torch.Tensor) -> torch.Tensor:
    """The logical NCHW (``channels_last``) view of an NHWC tensor."""
    return t.permute(0, 3, 1, 2)


def grad_nhwc(gy: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """The incoming NCHW gradient as the dense NHWC ``dtype`` tensor the kernels read: a view when it already is one."""
    g = nhwc(gy)
    if g.dtype != dtype or not g.is_contiguous():
        g = g.to(dtype).contiguous()
    return g
