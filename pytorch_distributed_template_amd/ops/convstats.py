"""BatchNorm statistics formed by the pointwise conv that produces the BatchNorm's input (``--native-convstats on``).

After ``convert_pointwise`` and ``convert_bnact``, a :class:`~.pointwise.PointwiseConv2d` directly followed by a
:class:`~.bnact.BNAct2d` inside an ``nn.Sequential`` is a pair: the conv runs ``pwconv_fwd_stats``, whose epilogue sums
``y`` and ``y**2`` per channel from the registers it stores ``y`` from, and the BatchNorm takes those fp64 slots instead
of reading the whole of ``y`` again in ``bnact_stats``.  The hand-over is a plain attribute on the tensor between the
two (``ops.bnact.CONV_STATS_ATTR``), checked against the tensor's version and removed by the BatchNorm; whenever it is
missing or stale (a hook that returned another tensor, an in-place change, eval mode, a fallback path) the BatchNorm
computes its statistics itself, as without this conversion.  No parameter, buffer, submodule or state-dict key changes.
"""
from __future__ import annotations

import torch.nn as nn

from . import bnact
from .bnact import BNAct2d
from .pointwise import PointwiseConv2d


def _hooked(m: nn.Module) -> bool:
    return bool(m._forward_hooks or m._forward_pre_hooks)


def convert_convstats(model: nn.Module) -> int:
    """Set ``emit_stats`` on every ``PointwiseConv2d`` at slot *i* of a plain ``nn.Sequential`` whose slot *i + 1* is a
    qualifying ``BNAct2d`` of the conv's output width, neither carrying forward (pre-)hooks.  Returns the number of
    pairs formed, 0 on a second call."""
    n = 0
    for parent in list(model.modules()):
        if not (isinstance(parent, nn.Sequential) and type(parent).forward is nn.Sequential.forward):
            continue
        children = list(parent._modules.values())  # every slot in order
        for conv, bn in zip(children, children[1:]):
            if (type(conv) is PointwiseConv2d and type(bn) is BNAct2d and not conv.emit_stats
                    and bn.num_features == conv.out_channels and bnact.qualifies(bn)
                    and not _hooked(conv) and not _hooked(bn)):
                conv.emit_stats = True
                n += 1
    return n
