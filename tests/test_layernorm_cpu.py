"""LayerNorm conversion (``ops/layernorm.py``) and the ``--native-layernorm`` flag without a GPU."""
import copy
import os
import subprocess
import sys

import pytest
import torch

from pytorch_distributed_template_amd.models import registry
from pytorch_distributed_template_amd.ops.layernorm import NativeLayerNorm, NativeLayerNorm2d, convert_layernorm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# convnext_tiny: 18 block + 1 stem + 3 downsample + 1 classifier; vit_b_16: 12 x 2 + the final norm; swin_t: 12 x 2 +
# the patch embedding + 3 patch mergings + the final norm
@pytest.mark.parametrize("arch,n", [("convnext_tiny", 23), ("vit_b_16", 25), ("swin_t", 29), ("resnet18", 0)])
def test_convert_counts(arch, n):
    model = registry.create(arch)
    assert convert_layernorm(model) == n
    assert sum(type(m) in (NativeLayerNorm, NativeLayerNorm2d) for m in model.modules()) == n
    assert convert_layernorm(model) == 0  # idempotent


def test_conversion_keeps_state_and_results():
    torch.manual_seed(0)
    model = registry.create("convnext_tiny").eval()
    ref = copy.deepcopy(model)
    keys, params = list(model.state_dict()), dict(model.named_parameters())
    names = [n for n, _ in model.named_modules()]
    assert convert_layernorm(model) == 23
    assert list(model.state_dict()) == keys and [n for n, _ in model.named_modules()] == names
    assert [n for n, _ in model.named_parameters()] == list(params)
    assert all(p is params[n] for n, p in model.named_parameters())  # the very same Parameter objects
    assert sum(type(m) is NativeLayerNorm2d for m in model.modules()) == 5
    x = torch.randn(2, 3, 32, 32)
    with torch.no_grad():
        assert torch.equal(model(x), ref(x))  # CPU: the modules fall back to F.layer_norm
    ref.load_state_dict(model.state_dict())


def test_cpu_run_logs_the_conversion(tmp_path):
    out = str(tmp_path / "out")
    args = ["dataparallel.py", "--outpath", out, "-a", "convnext_tiny", "-b", "2", "--synthetic", "--synthetic-train-size",
            "2", "--synthetic-val-size", "2", "--image-size", "32", "--num-classes", "10", "-j", "0", "--epochs", "1",
            "--iters-per-epoch", "1", "--val-iters", "1", "--exist-policy", "delete", "-p", "1", "--seed", "3",
            "--no-tensorboard", "--native-layernorm", "on"]
    env = dict(os.environ, PYTHONUNBUFFERED="1", OMP_NUM_THREADS="2", HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable] + args, cwd=ROOT, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    log = open(os.path.join(out + "_convnext_tiny", "experiment.log")).read()
    assert "=> native layernorm: 23 LayerNorm(s) of convnext_tiny converted" in log
