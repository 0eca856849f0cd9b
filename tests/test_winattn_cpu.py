"""Window-attention conversion (``ops/winattn.py``) and the ``--native-winattn`` flag without a GPU."""
import copy
import math
import types

import pytest
import torch

from pytorch_distributed_template_amd import cli
from pytorch_distributed_template_amd.models import modern, registry
from pytorch_distributed_template_amd.ops import conversions
from pytorch_distributed_template_amd.ops.winattn import (NativeRelPosAttention, NativeShiftedWindowAttention,
                                                          convert_window_attention)


# swin_t / swin_v2_t: 2 + 2 + 6 + 2 blocks; maxvit_t: (2 + 2 + 5 + 2) layers x (window + grid)
@pytest.mark.parametrize("arch,n", [("swin_t", 12), ("swin_v2_t", 12), ("maxvit_t", 22), ("resnet18", 0)])
def test_convert_counts_and_state(arch, n):
    model = registry.create(arch)
    keys, params = list(model.state_dict()), dict(model.named_parameters())
    assert sum(isinstance(m, (modern.ShiftedWindowAttention, modern.RelativePositionalMultiHeadAttention))
               for m in model.modules()) == n
    assert convert_window_attention(model) == n
    assert sum(type(m) in (NativeShiftedWindowAttention, NativeRelPosAttention) for m in model.modules()) == n
    assert list(model.state_dict()) == keys and [k for k, _ in model.named_parameters()] == list(params)
    assert all(p is params[k] for k, p in model.named_parameters())  # the very same Parameter objects
    assert convert_window_attention(model) == 0  # idempotent


@pytest.mark.parametrize("make,shape", [
    (lambda: modern.SwinTransformerBlock(96, 3, 7, 3, 0.0), (2, 14, 14, 96)),
    (lambda: modern.SwinTransformerBlock(64, 2, 8, 4, 0.0, v2=True), (1, 12, 16, 64)),  # padded to 16 x 16
    (lambda: modern.PartitionAttentionLayer(96, 32, 7, "grid", 14, 4, 0.0, 0.0, 0.0), (2, 96, 14, 14)),
])
def test_cpu_forward_is_the_parents(make, shape):
    torch.manual_seed(1)
    ref = make().train()
    nat = copy.deepcopy(ref)
    assert convert_window_attention(nat) == 1
    x = torch.randn(shape)
    assert torch.equal(nat(x), ref(x))


@pytest.mark.parametrize("Bw,heads,cap", [(3, 1, 512), (8, 3, 512), (5, 2, 512), (300, 3, 6), (300, 3, 3),
                                          (300, 3, 150), (128, 24, 1), (8192, 3, 512), (10 ** 6, 6, 512), (7, 5, 4)])
def test_plan_and_size_predicate(Bw, heads, cap):
    """The host-only bindings.  The counts decide the dbias summation order, so an edit must not move them."""
    from pytorch_distributed_template_amd.ops import native
    blocks, slabs = native.C.winattn_plan(Bw, heads, 49, cap)
    unit = heads // math.gcd(heads, 4)
    assert blocks * 4 == slabs * heads and blocks % unit == 0
    want = min(cap, -(-Bw * heads // 4))
    assert blocks == max(unit, want // unit * unit)
    assert all(native.C.winattn_fits(Bw, heads, N, 32) for N in (1, 49, 64))
    for bad in ((Bw, heads, 65, 32), (Bw, heads, 0, 32), (Bw, heads, 49, 64), (Bw, heads, 49, 16), (0, heads, 49, 32),
                (Bw, 0, 49, 32), (2 ** 31, heads, 49, 32)):
        assert not native.C.winattn_fits(*bad), bad
    with pytest.raises(RuntimeError):
        native.C.winattn_plan(Bw, heads, 65, cap)


def test_flag_parses_and_off_says_nothing():
    for mode in ("dp", "ddp", "ddp_amp"):
        p = cli.build_parser(mode)
        assert p.parse_args([]).native_winattn == "off"
        assert p.parse_args(["--native-winattn", "on"]).native_winattn == "on"
        assert "--native-winattn {off,on}" in p.format_help()
        with pytest.raises(SystemExit):
            p.parse_args(["--native-winattn", "auto"])
    lines = []
    model = registry.create("swin_t", num_classes=10)
    assert conversions.apply(model, types.SimpleNamespace(native_winattn="off"), "swin_t", False, lines.append) == {}
    assert lines == []
    got = conversions.apply(model, types.SimpleNamespace(native_winattn="on"), "swin_t", False, lines.append)
    assert got == {"winattn": (12,)} and lines == ["=> native winattn: 12 attention module(s) of swin_t converted"]
