"""Depthwise-conv module conversion and the ``--native-depthwise`` flag without a GPU: which convs of the registry
models qualify, that conversion keeps parameters / state dict / CPU results, and that a CPU run with the flag on
equals one with it off (every module falls back to ``F.conv2d`` there)."""
import copy
import io
import os
import pickle
import re
import subprocess
import sys

import pytest
import torch
import torch.nn as nn

from pytorch_distributed_template_amd import cli
from pytorch_distributed_template_amd.models import registry
from pytorch_distributed_template_amd.ops.depthwise import DepthwiseConv2d, convert_depthwise, qualifies

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# qualifying depthwise convs per registry model (ShuffleNetV2's 58- and 116-channel ones are no multiples of 8,
# ConvNeXt's are 7 x 7 with bias, ResNet has none)
COUNTS = [("mobilenet_v2", 17), ("mobilenet_v3_large", 15), ("mobilenet_v3_small", 11), ("mnasnet1_0", 17),
          ("efficientnet_b0", 16), ("shufflenet_v2_x1_0", 6), ("convnext_tiny", 0), ("resnet18", 0)]


@pytest.mark.parametrize("arch,count", COUNTS)
def test_convert_counts(arch, count):
    model = registry.create(arch)
    assert convert_depthwise(model) == count
    assert sum(isinstance(m, DepthwiseConv2d) for m in model.modules()) == count
    assert convert_depthwise(model) == 0  # idempotent


def test_qualifying_predicate():
    ok = nn.Conv2d(16, 16, 3, 1, 1, groups=16, bias=False)
    assert qualifies(ok)
    assert qualifies(nn.Conv2d(16, 16, 5, 2, 2, groups=16, bias=False))
    for bad in (nn.Conv2d(16, 16, 3, 1, 1, groups=16, bias=True), nn.Conv2d(16, 16, 3, 1, 1, groups=8, bias=False),
                nn.Conv2d(16, 32, 3, 1, 1, groups=16, bias=False), nn.Conv2d(16, 16, 7, 1, 3, groups=16, bias=False),
                nn.Conv2d(16, 16, 3, 1, 0, groups=16, bias=False), nn.Conv2d(16, 16, 3, 3, 1, groups=16, bias=False),
                nn.Conv2d(16, 16, 3, 1, 2, dilation=2, groups=16, bias=False),
                nn.Conv2d(16, 16, (3, 5), 1, (1, 2), groups=16, bias=False),
                nn.Conv2d(16, 16, 3, 1, 1, groups=16, bias=False, padding_mode="reflect"),
                nn.Conv2d(58, 58, 3, 1, 1, groups=58, bias=False)):
        assert not qualifies(bad), bad


def test_conversion_keeps_state_and_results():
    torch.manual_seed(0)
    model = registry.create("mobilenet_v2").eval()
    ref = copy.deepcopy(model)
    before = {k: v for k, v in model.state_dict().items()}
    params = {n: p for n, p in model.named_parameters()}
    hits = [n for n, m in model.named_modules() if isinstance(m, nn.Conv2d) and qualifies(m)]
    assert convert_depthwise(model) == 17
    after = model.state_dict()
    assert list(after.keys()) == list(before.keys())
    assert all(after[k] is before[k] or torch.equal(after[k], before[k]) for k in before)
    mods = dict(model.named_modules())
    for n in hits:
        assert type(mods[n]) is DepthwiseConv2d
        assert mods[n].weight is params[n + ".weight"]  # the very same Parameter object
        assert mods[n].weight.shape[1] == 1 and mods[n].bias is None
    assert [n for n, _ in model.named_parameters()] == list(params)
    # deep copy and pickle round trips keep the class and the values
    for clone in (copy.deepcopy(model), pickle.load(io.BytesIO(pickle.dumps(model)))):
        assert sum(isinstance(m, DepthwiseConv2d) for m in clone.modules()) == 17
        assert all(torch.equal(a, b) for a, b in zip(clone.state_dict().values(), after.values()))
    x = torch.randn(2, 3, 32, 32)
    with torch.no_grad():
        assert torch.equal(model(x), ref(x))  # CPU: every module falls back to F.conv2d
    # the state dict loads into an unconverted model and back
    ref.load_state_dict(model.state_dict())
    model.load_state_dict(ref.state_dict())


def test_module_constructor_and_cpu_gradients():
    torch.manual_seed(1)
    a = DepthwiseConv2d(16, 16, 3, stride=2, padding=1, groups=16, bias=False)
    b = nn.Conv2d(16, 16, 3, stride=2, padding=1, groups=16, bias=False)
    assert list(a.state_dict()) == list(b.state_dict()) and a.weight.shape == b.weight.shape == (16, 1, 3, 3)
    b.load_state_dict(a.state_dict())
    x = torch.randn(2, 16, 9, 7, requires_grad=True)
    x2 = x.detach().clone().requires_grad_(True)
    a(x).square().sum().backward()
    b(x2).square().sum().backward()
    assert torch.equal(a.weight.grad, b.weight.grad) and torch.equal(x.grad, x2.grad)


def test_flag_parses():
    for mode in ("dp", "ddp", "ddp_amp"):
        p = cli.build_parser(mode)
        assert p.parse_args([]).native_depthwise == "off"
        assert p.parse_args(["--native-depthwise", "on"]).native_depthwise == "on"
        assert p.parse_args(["--native-depthwise", "off"]).native_depthwise == "off"
        with pytest.raises(SystemExit):
            p.parse_args(["--native-depthwise", "auto"])


def _losses(tmp_path, flag):
    out = str(tmp_path / ("out_" + flag))
    args = ["dataparallel.py", "--outpath", out, "-a", "mobilenet_v2", "-b", "4", "--synthetic", "--synthetic-train-size",
            "8", "--synthetic-val-size", "4", "--image-size", "32", "--num-classes", "10", "-j", "0", "--epochs", "1",
            "--iters-per-epoch", "2", "--val-iters", "1", "--exist-policy", "delete", "-p", "1", "--seed", "3",
            "--no-tensorboard", "--native-depthwise", flag]
    env = dict(os.environ, PYTHONUNBUFFERED="1", OMP_NUM_THREADS="2", HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable] + args, cwd=ROOT, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    log = open(os.path.join(out + "_mobilenet_v2", "experiment.log")).read()
    return log, re.findall(r"Train epoch: \[0/1\]\[\d+/\d+\]\tlr=\S+\tce_loss=(\S+)\ttop1_acc=(\S+)", log)


def test_cpu_run_with_flag_on_equals_off(tmp_path):
    """Two iterations of mobilenet_v2 on CPU through the runner: the converted modules fall back to F.conv2d, so the
    loss lines are those of the unconverted run."""
    log_on, on = _losses(tmp_path, "on")
    log_off, off = _losses(tmp_path, "off")
    assert len(off) == 2 and on == off, (on, off)
    assert "=> native depthwise: 17 conv(s) of mobilenet_v2 converted" in log_on
    assert "native depthwise" not in log_off
