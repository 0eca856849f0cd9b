"""Global-attention conversion (``ops/mha.py``) and the ``--native-mha`` flag without a GPU."""
import copy
import types

import pytest
import torch

from pytorch_distributed_template_amd import cli
from pytorch_distributed_template_amd.models import modern, registry
from pytorch_distributed_template_amd.ops import conversions
from pytorch_distributed_template_amd.ops.mha import NativeMultiheadAttention, convert_mha


@pytest.mark.parametrize("arch,n", [("vit_b_16", 12), ("vit_b_32", 12), ("vit_l_16", 24), ("vit_l_32", 24),
                                    ("vit_h_14", 0), ("swin_t", 0), ("resnet18", 0)])  # vit_h_14: head dimension 80
def test_convert_counts_and_state(arch, n):
    model = registry.create(arch)
    keys, params = list(model.state_dict()), dict(model.named_parameters())
    assert convert_mha(model) == n
    assert sum(type(m) is NativeMultiheadAttention for m in model.modules()) == n
    assert list(model.state_dict()) == keys and [k for k, _ in model.named_parameters()] == list(params)
    assert all(p is params[k] for k, p in model.named_parameters())  # the very same Parameter objects
    assert convert_mha(model) == 0  # idempotent


def test_cpu_forward_is_the_parents():
    torch.manual_seed(1)
    ref = modern.EncoderBlock(2, 128, 256, 0.0, 0.0).train()
    nat = copy.deepcopy(ref)
    assert convert_mha(nat) == 1
    x = torch.randn(3, 50, 128)
    assert torch.equal(nat(x), ref(x))


def test_size_predicate():
    from pytorch_distributed_template_amd.ops import native
    assert all(native.C.mha_fits(128, 12, N, 64) for N in (1, 50, 197, 4096))
    for bad in ((128, 12, 0, 64), (128, 12, 4097, 64), (128, 12, 197, 32), (128, 12, 197, 80), (128, 0, 197, 64),
                (0, 12, 197, 64), (2 ** 30, 16, 4096, 64)):
        assert not native.C.mha_fits(*bad), bad


def test_flag_parses_and_off_says_nothing():
    for mode in ("dp", "ddp", "ddp_amp"):
        p = cli.build_parser(mode)
        assert p.parse_args([]).native_mha == "off"
        assert p.parse_args(["--native-mha", "on"]).native_mha == "on"
        assert "--native-mha {off,on}" in p.format_help()
        with pytest.raises(SystemExit):
            p.parse_args(["--native-mha", "auto"])
    lines = []
    model = registry.create("vit_b_16", num_classes=10)
    assert conversions.apply(model, types.SimpleNamespace(native_mha="off"), "vit_b_16", False, lines.append) == {}
    assert lines == []
    got = conversions.apply(model, types.SimpleNamespace(native_mha="on"), "vit_b_16", False, lines.append)
    assert got == {"mha": (12,)} and lines == ["=> native mha: 12 attention module(s) of vit_b_16 converted"]
