"""GELU-MLP conversion (``ops/mlp.py``), the host-side plan and the ``--native-mlp`` flag without a GPU."""
import types

import pytest
import torch
import torch.nn as nn

from pytorch_distributed_template_amd import cli
from pytorch_distributed_template_amd.models import registry
from pytorch_distributed_template_amd.ops import conversions, mlp


def test_flag_parses():
    for mode in ("dp", "ddp", "ddp_amp"):
        p = cli.build_parser(mode)
        assert p.parse_args([]).native_mlp == "off"
        assert p.parse_args(["--native-mlp", "on"]).native_mlp == "on"
        assert "--native-mlp {off,on}" in p.format_help()
        with pytest.raises(SystemExit):
            p.parse_args(["--native-mlp", "auto"])


# the last stage of ConvNeXt and Swin and every ViT block have Hd = 3072: outside the contract
@pytest.mark.parametrize("arch,n", [("convnext_tiny", 15), ("swin_t", 10), ("vit_b_16", 0)])
def test_apply_counts_and_state(arch, n):
    model = registry.create(arch, num_classes=10)
    keys, params, kinds = list(model.state_dict()), dict(model.named_parameters()), [type(m) for m in model.modules()]
    lines = []
    got = conversions.apply(model, types.SimpleNamespace(native_mlp="on"), arch, False, lines.append)
    assert got == {"mlp": (n,)} and lines == [f"=> native mlp: {n} MLP(s) of {arch} converted"]
    after = list(model.modules())
    # one run per converted parent; every other module keeps its class, a parent becomes a subclass of its own
    assert sum(type(m) in mlp.KINDS.values() for m in after) == n
    assert all(type(m) is k or mlp.KINDS.get(k) is type(m) for m, k in zip(after, kinds)) and len(after) == len(kinds)
    assert list(model.state_dict()) == keys and [k for k, _ in model.named_parameters()] == list(params)
    assert all(p is params[k] for k, p in model.named_parameters())  # the very same Parameter objects
    assert mlp.convert_mlp(model) == 0  # idempotent


def test_maxvit_converts_every_mlp_layer():
    model = registry.create("maxvit_t", num_classes=10)
    n = sum(name.endswith("mlp_layer") for name, _ in model.named_modules())
    assert n > 0 and mlp.convert_mlp(model) == n
    assert all(type(m) is mlp.NativeMLPSequential for name, m in model.named_modules() if name.endswith("mlp_layer"))


def test_cpu_forward_is_the_stock_one():
    torch.manual_seed(0)
    ref = registry.create("convnext_tiny", num_classes=10).eval()
    torch.manual_seed(0)
    nat = registry.create("convnext_tiny", num_classes=10).eval()
    assert mlp.convert_mlp(nat) == 15
    x = torch.randn(2, 3, 64, 64)
    with torch.no_grad():
        assert torch.equal(nat(x), ref(x))


def _seq(*mods):
    return nn.Sequential(nn.Sequential(*mods))


def test_hooked_or_unlisted_runs_stay():
    hooked = _seq(nn.Linear(8, 32), nn.GELU(), nn.Linear(32, 8))
    hooked[0][1].register_forward_hook(lambda m, i, o: None)
    others = [hooked, _seq(nn.Linear(8, 32), nn.GELU(approximate="tanh"), nn.Linear(32, 8)),
              _seq(nn.Linear(8, 32, bias=False), nn.GELU(), nn.Linear(32, 8)),
              _seq(nn.Linear(8, 32), nn.GELU(), nn.Linear(16, 8)), _seq(nn.Linear(96, 3072), nn.GELU(), nn.Linear(3072, 96))]
    for model in others:
        assert mlp.convert_mlp(model) == 0 and type(model[0]) is nn.Sequential
    two = _seq(nn.LayerNorm(8), nn.Linear(8, 32), nn.GELU(), nn.Dropout(0.1), nn.Linear(32, 8), nn.Linear(8, 16), nn.GELU(),
               nn.Linear(16, 8))
    assert mlp.convert_mlp(two) == 2 and type(two[0]) is mlp.NativeMLPSequential


def test_size_predicate_and_plan():
    for ok in ((1, 8, 8, 8), (2 ** 30, 512, 2048, 512), (517, 24, 40, 24)):
        assert mlp.mlp_fits(*ok), ok
    for bad in ((0, 8, 8, 8), (2 ** 30 + 1, 8, 8, 8), (1, 520, 2048, 512), (1, 512, 2056, 512), (1, 96, 3072, 96),
                (1, 96, 384, 520), (1, 12, 48, 12), (1, 8, 8, 0)):
        assert not mlp.mlp_fits(*bad), bad
    # (splits, rows per split, Hd tiles, Co tiles, chain = 2 * (rows per split + 4 waves + splits)): pinned, they fix
    # the summation order
    assert mlp.mlp_fc2_wgrad_plan(517, 40, 24, 2) == (2, 384, 1, 1, 780)
    assert mlp.mlp_fc2_wgrad_plan(517, 384, 96, 36) == (3, 256, 6, 2, 526)
    assert mlp.mlp_fc2_wgrad_plan(128 * 3136, 384, 96) == (85, 4736, 6, 2, 2 * (4736 + 4 + 85))
