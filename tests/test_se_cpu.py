"""Squeeze-and-excitation conversion (``ops/se.py``), the host-side plan and the ``--native-se`` flag without a GPU."""
import copy
import types

import pytest
import torch
import torch.nn as nn

from pytorch_distributed_template_amd import cli
from pytorch_distributed_template_amd.models import efficient, modern, registry
from pytorch_distributed_template_amd.ops import conversions, native, se


@pytest.mark.parametrize("arch,n", [("efficientnet_b0", 16), ("efficientnet_v2_s", 30), ("mobilenet_v3_large", 8),
                                    ("mobilenet_v3_small", 9), ("regnet_y_400mf", 16), ("maxvit_t", 11),
                                    ("regnet_x_400mf", 0), ("resnet18", 0)])
def test_convert_counts_and_state(arch, n):
    model = registry.create(arch)
    keys, params = list(model.state_dict()), dict(model.named_parameters())
    assert se.convert_se(model) == n
    assert sum(type(m) in se.KINDS.values() for m in model.modules()) == n
    assert list(model.state_dict()) == keys and [k for k, _ in model.named_parameters()] == list(params)
    assert all(p is params[k] for k, p in model.named_parameters())  # the very same Parameter objects
    assert se.convert_se(model) == 0  # idempotent


@pytest.mark.parametrize("make,cls", [
    (lambda: efficient.SqueezeExcitation(24, 8), se.NativeSqueezeExcitation),
    (lambda: efficient.SqueezeExcitation(24, 6, nn.SiLU, nn.Sigmoid), se.NativeSqueezeExcitation),
    (lambda: modern._RegNetSE(104, 26), se.NativeRegNetSE), (lambda: modern._SE(64, 16), se.NativeSE)])
def test_cpu_forward_is_the_parents(make, cls):
    torch.manual_seed(1)
    ref = nn.Sequential(make())
    nat = copy.deepcopy(ref)
    assert se.convert_se(nat) == 1 and type(nat[0]) is cls
    x = torch.randn(3, ref[0].fc1.in_channels, 5, 7)
    assert torch.equal(nat(x), ref(x))


def test_hooked_or_unlisted_modules_stay():
    hooked = nn.Sequential(modern._RegNetSE(16, 4))
    hooked[0].fc2.register_forward_hook(lambda m, i, o: None)
    pre = nn.Sequential(modern._RegNetSE(16, 4))
    pre[0].activation.register_forward_pre_hook(lambda m, i: None)
    gelu = nn.Sequential(efficient.SqueezeExcitation(16, 4, nn.GELU, nn.Sigmoid))
    odd = nn.Sequential(efficient.SqueezeExcitation(12, 4))  # C % 8 != 0
    for model in (hooked, pre, gelu, odd):
        assert se.convert_se(model) == 0 and type(model[0]) not in se.KINDS.values()


def test_size_predicate():
    for ok in ((1, 1, 8, 1), (400, 12544, 32, 8), (2, 49, 4096, 512)):
        assert native.C.se_fits(*ok), ok
    for bad in ((1, 49, 12, 4), (1, 49, 4104, 4), (1, 49, 32, 0), (1, 49, 32, 513), (1, 0, 32, 8), (0, 49, 32, 8),
                (2 ** 20, 2 ** 10, 1024, 8), (2 ** 62, 2 ** 62, 8, 8)):
        assert not native.C.se_fits(*bad), bad


# (N, HW, C, cap) -> (chunks, rows_per_chunk): pinned, they fix the summation order.  A block is C / 8 channel groups x
# 256 // (C / 8) row lanes; a chunk has at least 8 rows per row lane and 64 rows, unless the cap leaves the image fewer
@pytest.mark.parametrize("args,plan", [
    ((1, 1, 8, 2048), (1, 1)), ((400, 49, 1152, 2048), (1, 49)), ((2, 3136, 32, 2048), (7, 448)),
    ((2, 3136, 32, 1), (1, 3136)), ((128, 12544, 32, 2048), (16, 784)), ((400, 12544, 32, 2048), (5, 2509)),
    ((3000, 196, 480, 2048), (1, 196)), ((8, 784, 144, 2048), (7, 112)), ((1, 7, 4096, 2048), (1, 7))])
def test_plan(args, plan):
    N, HW, C, cap = args
    chunks, rpc = native.C.se_plan(*args)
    assert chunks >= 1 and chunks * rpc >= HW > (chunks - 1) * rpc and (N > cap or N * chunks <= cap)
    assert (chunks, rpc) == plan and se.se_plan(N, HW, C, cap) == plan


def test_flag_parses_and_off_says_nothing():
    for mode in ("dp", "ddp", "ddp_amp"):
        p = cli.build_parser(mode)
        assert p.parse_args([]).native_se == "off"
        assert p.parse_args(["--native-se", "on"]).native_se == "on"
        assert "--native-se {off,on}" in p.format_help()
        with pytest.raises(SystemExit):
            p.parse_args(["--native-se", "auto"])
    lines = []
    model = registry.create("efficientnet_b0", num_classes=10)
    assert conversions.apply(model, types.SimpleNamespace(native_se="off"), "efficientnet_b0", False, lines.append) == {}
    assert lines == []
    got = conversions.apply(model, types.SimpleNamespace(native_se="on"), "efficientnet_b0", False, lines.append)
    assert got == {"se": (16,)}
    assert lines == ["=> native se: 16 squeeze-excitation module(s) of efficientnet_b0 converted"]
