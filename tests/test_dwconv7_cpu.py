"""7x7 depthwise conv conversion (``ops/depthwise7.py``) and the ``--native-dw7`` flag without a GPU."""
import copy

import pytest
import torch
import torch.nn as nn

from pytorch_distributed_template_amd.models import registry
from pytorch_distributed_template_amd.ops.depthwise import convert_depthwise
from pytorch_distributed_template_amd.ops.depthwise7 import DepthwiseConv7x7, convert_depthwise7, qualifies7


@pytest.mark.parametrize("arch,n", [("convnext_tiny", 18), ("convnext_small", 36), ("mobilenet_v2", 0), ("resnet18", 0)])
def test_convert_counts(arch, n):
    model = registry.create(arch)
    assert convert_depthwise7(model) == n
    assert sum(type(m) is DepthwiseConv7x7 for m in model.modules()) == n
    assert convert_depthwise7(model) == 0  # idempotent
    if arch == "convnext_tiny":
        assert convert_depthwise(model) == 0  # the 3x3 / 5x5 converter still finds nothing


def test_conversion_keeps_state_and_results():
    torch.manual_seed(0)
    model = registry.create("convnext_tiny").eval()
    ref = copy.deepcopy(model)
    keys, params = list(model.state_dict()), dict(model.named_parameters())
    names = [n for n, _ in model.named_modules()]
    hits = [n for n, m in model.named_modules() if isinstance(m, nn.Conv2d) and qualifies7(m)]
    assert convert_depthwise7(model) == 18 == len(hits)
    assert list(model.state_dict()) == keys and [n for n, _ in model.named_modules()] == names
    mods = dict(model.named_modules())
    for h in hits:  # the very same Parameter objects, bias included
        assert mods[h].weight is params[h + ".weight"] and mods[h].bias is params[h + ".bias"]
    assert [n for n, _ in model.named_parameters()] == list(params)
    x = torch.randn(2, 3, 32, 32)
    with torch.no_grad():
        assert torch.equal(model(x), ref(x))  # CPU: the modules fall back to F.conv2d
    ref.load_state_dict(model.state_dict())


@pytest.mark.parametrize("kw,want", [
    (dict(), True),
    (dict(bias=False), True),
    (dict(c=8), True),
    (dict(c=60), False),           # C % 8
    (dict(k=5, padding=2), False),
    (dict(stride=2), False),
    (dict(padding=2), False),
    (dict(dilation=2, padding=6), False),
    (dict(groups=8), False),       # grouped, not depthwise
    (dict(padding_mode="reflect"), False),
])
def test_qualifies7(kw, want):
    kw = dict(kw)
    c, k = kw.pop("c", 96), kw.pop("k", 7)
    kw.setdefault("padding", 3)
    kw.setdefault("groups", c)
    assert qualifies7(nn.Conv2d(c, c, k, **kw)) is want
