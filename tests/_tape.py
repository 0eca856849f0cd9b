"""Recording proxy for the native extension module (a plain module, not a conftest).

``ex.C = Tape(ex.C)`` makes every kernel launch of a ResNetExecutor or VGGExecutor step (and ``monkeypatch.setattr(native, "C",
Tape(native.C))`` every launch of the torch engine's converted modules, which read ``native.C.<name>`` at call time:
tests/_torch_audit.py) leave an entry
``Call(index, name, args, kwargs, outs, ret)`` on ``tape.calls``: ``outs`` maps the argument position (or keyword name)
of every tensor the launcher WRITES to a clone taken right after the call (the device is synchronised first, so with the
executor on one stream -- PDT_WGRAD_STREAM=0 -- the clone holds what the kernel wrote); ``ret`` is what the launcher
returned (the ``(blocks, lanes)`` of the reduce passes, the splits of a weight gradient).  The arguments themselves are
kept by reference: ``value_at`` resolves what an input tensor held at the time of a call from the latest earlier write
to the same address, or, where the step never wrote it through the tape, from the live tensor.

Which arguments a launcher writes is ``WRITES`` below: launcher name -> argument indices / keyword names.  ``()`` is an
op no audit reads an output of.  A name that is neither there nor a query raises: a launch added to the step cannot go
unrecorded silently.
"""
from collections import namedtuple

import torch

Call = namedtuple("Call", "index name args kwargs outs ret")

# launcher -> positions (or keyword names) of the tensors it writes (csrc/bindings.cpp signatures)
WRITES = {
    "stem_pack": (1,), "stem_pack_u8": (1,),
    "stem_fwd": (2, 3),                       # y, statistics slots
    "conv_fwd": (2, 4), "conv1x1_c64": (2, 3), "conv_fwd_pre": (2, 3), "conv1x1x": (2, 3), "gconv_fwd": (2, 3),
    "bn_finalize_slots": (6, 7, 8, 9),        # running_mean, running_var, coef, sums
    "bn_slot_sum": (3,),
    "bn_finalize": (6, 7, 8),
    "bn_eval_coef": (5,),
    "bn_apply": (4, 8),                       # out, ReLU bitmask
    "bn_relu_maxpool": (2, 3),                # pooled out, argmax
    "avgpool_fwd": (1,), "avgpool_bwd": (1,),
    "xent": (6, 7, 10, 11),                   # fp32 logits, dlogits, row loss, row correct
    "metrics": (3,),
    "colsum": (4,),
    "conv_wgrad": (), "conv_wgrad_3x3c64": (), "gconv_wgrad": (), "gconv_wgrad_l1": (), "conv_wgrad_stem_fused": (),
    "wgrad_reduce": (6,),
    "gather32": (2,), "gather16": (2,),
    "bn_bwd_reduce": (6,),
    "bn_bwd_finalize_slots": (5, 6, 7, 10, 11, 12),  # dgamma1, dbeta1, bcoef1, dgamma2, dbeta2, bcoef2
    "bn_bwd_finalize": (4, 5, 7),             # dgamma, dbeta, bcoef
    "bn_bwd_apply": (4, 7, 8),                # dy1, dy2, dz
    "conv_dgrad": (2,),
    "conv_dgrad_bn": (2, 22),                 # dx, BN-backward slots
    "gconv_dgrad": (2, "bn_slots"),
    "stem_pool_bwd_reduce_out": (3,),
    "stem_pool_bwd_apply": (5,),
    # the torch engine's converted modules (ops/bnact.py, depthwise.py, pointwise.py, stemconv.py)
    "bnact_stats": (1,), "bnact_fwd": (2,), "bnact_bwd_reduce": (3,), "bnact_bwd_apply": (4,),  # slots, out, slots, dx
    "dwconv_fwd": (2,), "dwconv_dgrad": (2,), "dwconv_wgrad": (2,),                             # y, dx, ws
    "pwconv_fwd": (2,), "pwconv_dgrad": (2,), "pwconv_wgrad": (2,),
    "stem3x3_fwd": (2,), "stem3x3_wgrad": (2,),
    # the VGG / AlexNet executor (models/executor_vgg.py, csrc/kernels/vgg.hip); its classifier GEMMs are torch.mm(out=)
    # outside the extension: tests/_vgg_audit.py takes those from ``saved`` and the executor's buffers
    "bias_coef": (1,),
    "bn_relu_maxpool2": (2, 3),               # pooled out, argmax (None in eval)
    "maxpool2_bwd": (5,), "maxpool_bwd_relu": (4,),
    "pooled_bwd_reduce": (3,),                # BN-backward slots
    "fc_act_fwd": (2,), "fc_act_bwd": (2,),
    "nhwc_nchw16": (1,),
    "sgd": (),                                # TorchTrainer's optimizer update goes through native.C too: not audited
}

_QUERY_SUFFIX = ("_supported", "_plan", "_blocks", "_mode", "_fits")
_QUERIES = {"stat_slots", "conv_dgrad_persistent", "dispatch_counts", "reset_dispatch_counts", "wgrad_blocks_3x3c64",
            "conv_m_tiles", "gconv_slice"}


def is_query(name):
    return name in _QUERIES or name.endswith(_QUERY_SUFFIX)


def _sync(t):
    if t.is_cuda:
        torch.cuda.synchronize(t.device)


class Tape:
    def __init__(self, module, writes=None):
        self._mod = module
        self._writes = WRITES if writes is None else writes
        self.calls = []

    def __getattr__(self, name):
        fn = getattr(self._mod, name)  # AttributeError for a launcher the build lacks: hasattr() keeps working
        if is_query(name) or not callable(fn):
            return fn
        if name not in self._writes:
            raise KeyError(f"Tape: launcher `{name}` has no entry in tests/_tape.py WRITES: say what it writes, so the "
                           "step audit can judge it")
        where = self._writes[name]

        def recorded(*args, **kwargs):
            ret = fn(*args, **kwargs)
            outs = {}
            for k in where:
                t = kwargs.get(k) if isinstance(k, str) else (args[k] if k < len(args) else None)
                if torch.is_tensor(t):
                    _sync(t)
                    outs[k] = t.detach().clone()
            self.calls.append(Call(len(self.calls), name, args, kwargs, outs, ret))
            return ret
        recorded.__name__ = name
        return recorded

    # ------------------------------------------------------------------------------------------------ lookups
    def clear(self):
        self.calls = []

    def named(self, *names):
        return [c for c in self.calls if c.name in names]

    def count(self, name):
        return sum(1 for c in self.calls if c.name == name)

    def value_at(self, index, t):
        """What tensor ``t`` (an argument of call ``index``) held when that call started."""
        if t is None:
            return None
        ptr, n = t.data_ptr(), t.numel()
        for c in reversed(self.calls[:index]):
            for k, o in c.outs.items():
                w = c.kwargs.get(k) if isinstance(k, str) else c.args[k]
                if w.data_ptr() == ptr and w.dtype == t.dtype and o.numel() >= n:
                    return o.reshape(-1)[:n].view(t.shape)
        return t

    def find(self, name, **match):
        """Calls ``name`` whose argument at position / keyword k IS the tensor given (same address and size)."""
        out = []
        for c in self.named(name):
            ok = True
            for k, t in match.items():
                k = int(k[1:]) if k[0] == "a" and k[1:].isdigit() else k
                a = c.kwargs.get(k) if isinstance(k, str) else (c.args[k] if k < len(c.args) else None)
                if not (torch.is_tensor(a) and a.data_ptr() == t.data_ptr() and a.numel() == t.numel()):
                    ok = False
            if ok:
                out.append(c)
        return out
