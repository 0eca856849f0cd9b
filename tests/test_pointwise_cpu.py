"""Pointwise-conv cases, module conversion and the ``--native-pointwise`` flag without a GPU.

* the cases of tests/_pointwise_cases.py are proven before any kernel runs: the layer-A condition holds on every
  reference, and a torch emulation of a correct kernel (a plain fp32 matmul rounded once) passes both layers;
* mutations of that emulation -- a dropped reduction chunk, a reduction that runs into the next pixel, a dropped pixel
  row, output channels shifted by 8, one 16-bit ulp, truncation, a weight gradient without its last split -- each fail
  the same check;
* which convs of the registry models qualify, that conversion keeps parameters / state dict / CPU results, the flag,
  and a CPU run with the flag on equals one with it off (every module falls back to ``F.conv2d`` there).
"""
import copy
import itertools
import os
import re
import subprocess
import sys

import pytest
import torch
import torch.nn as nn

import _numerics as nm
import _pointwise_cases as pc
from pytorch_distributed_template_amd import cli
from pytorch_distributed_template_amd.models import registry
from pytorch_distributed_template_amd.ops.pointwise import PointwiseConv2d, convert_pointwise, qualifies

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

COUNTS = [("mobilenet_v2", 34), ("mnasnet1_0", 34), ("mobilenet_v3_large", 30), ("mobilenet_v3_small", 22),
          ("efficientnet_b0", 32), ("shufflenet_v2_x1_0", 10), ("densenet121", 61),
          ("resnet50", 33),       # its three stride-2 downsample convs stay
          ("squeezenet1_1", 0)]   # all biased

GD = [(g, dt) for g in pc.GEOMS for dt in pc.DTYPES]
_ids = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v).split(".")[-1]


# ------------------------------------------------------------------------------ the cases, on references alone
@pytest.mark.parametrize("g,dtype", GD, ids=_ids)
def test_layer_a_conditions(g, dtype):
    """Integer outputs are (all but 1 %) exactly representable in the 16-bit type; every partial sum of the weight
    gradient is an integer far below 2**24."""
    N, H, W, C, K = g
    assert nm.int_case_conditions(pc.case("fwd", g, dtype, "int")["ref"], dtype, K)[0] <= 0.01
    assert nm.int_case_conditions(pc.case("dgrad", g, dtype, "int")["ref"], dtype, C)[0] <= 0.01
    assert pc.case("wgrad", g, dtype, "int")["mag"].max().item() < 2.0 ** 20


@pytest.mark.parametrize("layer", pc.LAYERS)
@pytest.mark.parametrize("g,dtype", GD, ids=_ids)
def test_emulation_passes(g, dtype, layer):
    d = pc.case("fwd", g, dtype, layer)
    pc.judge(pc.emul_fwd(d["x"], d["w"], dtype), d, dtype, layer, f"fwd {g}", None)
    d = pc.case("dgrad", g, dtype, layer)
    pc.judge(pc.emul_dgrad(d["dy"], d["w"], dtype), d, dtype, layer, f"dgrad {g}", None)
    d = pc.case("wgrad", g, dtype, layer)
    for pps in (128, 1 << 20):
        pc.judge_dw(pc.emul_wgrad(d["x"], d["dy"], pps), d, layer, f"wgrad {g}", None)


# ------------------------------------------------------------------------------ mutations must fail the same check
def _fwd_like(kind, g, dtype, layer):
    """(activation [rows, R], weight as [out, R], the emulation's output [rows, out]) of a forward / backward-data case."""
    d = pc.case(kind, g, dtype, layer)
    if kind == "fwd":
        a, b = d["x"], d["w"]
    else:
        a, b = d["dy"], d["w"].t().contiguous()
    a2 = a.reshape(-1, a.shape[-1])
    return d, a2, b, (a2.float() @ b.float().t())


def _rejected(out32, d, dtype, layer, name):
    with pytest.raises(AssertionError):
        pc.judge(out32.to(dtype).reshape(d["ref"].shape), d, dtype, layer, name, None)


@pytest.mark.parametrize("layer", pc.LAYERS)
@pytest.mark.parametrize("kind", ["fwd", "dgrad"])
@pytest.mark.parametrize("g,dtype", GD, ids=_ids)
def test_structural_mutations_fail(g, dtype, kind, layer):
    d, a, b, good = _fwd_like(kind, g, dtype, layer)
    rows, R = a.shape
    nout = b.shape[0]
    af, bf = a.float(), b.float()
    # the last 8 reduction channels dropped (a reduction tail masked one chunk early)
    _rejected(af[:, :R - 8] @ bf[:, :R - 8].t(), d, dtype, layer, "dropped reduction chunk")
    # the reduction runs 8 channels into the next pixel's row (an unmasked tail chunk) against live weights
    if rows > 1:
        nxt = torch.cat([af[1:, :8], torch.zeros(1, 8)])
        _rejected(good + nxt @ bf[:, :8].t(), d, dtype, layer, "reduction padded with the next pixel")
    # the last pixel row never written (an output buffer of zeros)
    out = good.clone()
    out[-1] = 0
    _rejected(out, d, dtype, layer, "dropped pixel row")
    # output channel k taken from k + 8 (a fragment-row permutation off by one group)
    if nout > 8:
        out = good.clone()
        out[:, :nout - 8] = good[:, 8:]
        _rejected(out, d, dtype, layer, "output channels shifted by 8")


def _next16(t, dtype):
    """Every element moved one 16-bit ulp away from zero."""
    return (t.to(dtype).view(torch.int16) + 1).view(dtype)


@pytest.mark.parametrize("kind", ["fwd", "dgrad"])
@pytest.mark.parametrize("g,dtype", GD, ids=_ids)
def test_one_ulp_fails_layer_a(g, dtype, kind):
    d, a, b, good = _fwd_like(kind, g, dtype, "int")
    with pytest.raises(AssertionError):
        pc.judge(_next16(good, dtype).reshape(d["ref"].shape), d, dtype, "int", "one ulp", None)


# Rounding mutations in layer B are visible where the 16-bit half ulp dominates the bound: reductions of at most 40
# terms ((n + 4) * 2u * mag <= 44 * 2^-23 * mag, far below the 2^-9 / 2^-12 relative half ulp for mag ~ |ref|).
SHORT = [(kind, g) for g in pc.GEOMS for kind in ("fwd", "dgrad") if (g[3] if kind == "fwd" else g[4]) <= 40]


@pytest.mark.parametrize("dtype", pc.DTYPES, ids=_ids)
@pytest.mark.parametrize("kind,g", SHORT, ids=_ids)
def test_rounding_mutations_fail_layer_b(kind, g, dtype):
    d, a, b, good = _fwd_like(kind, g, dtype, "real")
    with pytest.raises(AssertionError):
        pc.judge(_next16(good, dtype).reshape(d["ref"].shape), d, dtype, "real", "one ulp", None)
    # truncation instead of rounding: the 16 low bits of the fp32 value (bf16) / round toward zero (fp16)
    if dtype == torch.bfloat16:
        trunc = (good.view(torch.int32) & -65536).view(torch.float32).to(dtype)
    else:
        r = good.to(dtype)
        over = r.float().abs() > good.abs()
        trunc = torch.where(over, (r.view(torch.int16) - 1).view(dtype), r)
    with pytest.raises(AssertionError):
        pc.judge(trunc.reshape(d["ref"].shape), d, dtype, "real", "truncation", None)


@pytest.mark.parametrize("layer", pc.LAYERS)
@pytest.mark.parametrize("g,dtype", GD, ids=_ids)
def test_wgrad_missing_split_fails(g, dtype, layer):
    d = pc.case("wgrad", g, dtype, layer)
    with pytest.raises(AssertionError):
        pc.judge_dw(pc.emul_wgrad(d["x"], d["dy"], 128, drop_last_split=True), d, layer, "missing split", None)


@pytest.mark.parametrize("g", pc.TINY_GEOMS, ids=_ids)
def test_tiny_layer_emulation_passes_and_mutations_fail(g):
    """fp16 weight gradient with subnormal dY (the ``real`` operand times 2**-16), judged over the nominal magnitudes: the
    emulation stays inside the bound; a missing split, a dropped pixel and gradient rows shifted by one output channel
    leave it."""
    dt = torch.float16
    N, H, W, C, K = g
    d = pc.case("wgrad", g, dt, "tiny")
    a = d["dy"].float().abs()
    # subnormal and nonzero: all but the |dy| >= 4 and the |dy| < 2**-9 of a normal sample
    assert float((a < nm.FP16_MIN_NORMAL).float().mean()) > 0.999 and float((a > 0).float().mean()) > 0.99
    assert torch.equal(d["x"], pc.case("wgrad", g, dt, "real")["x"])
    plain = nm.conv_wgrad_ref(d["x"], d["dy"], 1, 1, 1, 0)[1].reshape(K, C)
    assert bool((d["mag"] >= plain).all()) and bool((d["mag"] > plain).any())
    for pps in (128, 1 << 20):
        pc.judge_dw(pc.emul_wgrad(d["x"], d["dy"], pps), d, "tiny", f"tiny wgrad {g}", None)
    good = pc.emul_wgrad(d["x"], d["dy"], 128)
    cut = d["dy"].clone()
    cut.view(-1, K)[-1] = 0
    for name, bad in (("missing split", pc.emul_wgrad(d["x"], d["dy"], 128, drop_last_split=True)),
                      ("dropped pixel", pc.emul_wgrad(d["x"], cut, 128)), ("rows shifted by one", good.roll(1, 0))):
        with pytest.raises(AssertionError):
            pc.judge_dw(bad, d, "tiny", name, None)


# ------------------------------------------------------------------------------ module conversion
@pytest.mark.parametrize("arch,count", COUNTS)
def test_convert_counts(arch, count):
    model = registry.create(arch)
    assert convert_pointwise(model) == count
    assert sum(isinstance(m, PointwiseConv2d) for m in model.modules()) == count
    assert convert_pointwise(model) == 0  # idempotent


def test_qualifying_predicate():
    assert qualifies(nn.Conv2d(16, 96, 1, bias=False))
    assert qualifies(nn.Conv2d(8, 2048, 1, bias=False)) and qualifies(nn.Conv2d(2048, 8, 1, bias=False))
    for bad in (nn.Conv2d(16, 96, 1, bias=True), nn.Conv2d(16, 96, 1, stride=2, bias=False),
                nn.Conv2d(16, 96, 1, padding=1, bias=False), nn.Conv2d(16, 96, 1, groups=2, bias=False),
                nn.Conv2d(16, 96, 3, padding=1, bias=False), nn.Conv2d(16, 96, (1, 3), padding=(0, 1), bias=False),
                nn.Conv2d(16, 96, 1, dilation=2, bias=False), nn.Conv2d(58, 96, 1, bias=False),
                nn.Conv2d(16, 100, 1, bias=False), nn.Conv2d(4, 8, 1, bias=False), nn.Conv2d(16, 2056, 1, bias=False),
                nn.Conv2d(2056, 16, 1, bias=False)):
        assert not qualifies(bad), bad


def test_conversion_keeps_state_and_results():
    torch.manual_seed(0)
    model = registry.create("mobilenet_v2").eval()
    ref = copy.deepcopy(model)
    before = dict(model.state_dict())
    params = dict(model.named_parameters())
    hits = [n for n, m in model.named_modules() if isinstance(m, nn.Conv2d) and qualifies(m)]
    assert convert_pointwise(model) == 34 == len(hits)
    after = model.state_dict()
    assert list(after.keys()) == list(before.keys())
    assert all(after[k] is before[k] or torch.equal(after[k], before[k]) for k in before)
    mods = dict(model.named_modules())
    for n in hits:
        assert type(mods[n]) is PointwiseConv2d
        assert mods[n].weight is params[n + ".weight"]  # the very same Parameter object
    assert [n for n, _ in model.named_parameters()] == list(params)
    assert convert_pointwise(model) == 0
    x = torch.randn(2, 3, 32, 32)
    with torch.no_grad():
        assert torch.equal(model(x), ref(x))  # CPU: every module falls back to F.conv2d
    ref.load_state_dict(model.state_dict())
    model.load_state_dict(ref.state_dict())


def test_three_converters_in_every_order():
    from pytorch_distributed_template_amd.ops.bnact import convert_bnact
    from pytorch_distributed_template_amd.ops.depthwise import convert_depthwise
    base = registry.create("mobilenet_v2")
    conv = {"pointwise": convert_pointwise, "depthwise": convert_depthwise, "bnact": convert_bnact}
    want = {"pointwise": 34, "depthwise": 17, "bnact": (52, 35)}
    for order in itertools.permutations(conv):
        m = copy.deepcopy(base)
        assert {k: conv[k](m) for k in order} == want, order


def test_module_constructor_and_cpu_gradients():
    torch.manual_seed(1)
    a = PointwiseConv2d(16, 24, 1, bias=False)
    b = nn.Conv2d(16, 24, 1, bias=False)
    assert list(a.state_dict()) == list(b.state_dict()) and a.weight.shape == b.weight.shape == (24, 16, 1, 1)
    b.load_state_dict(a.state_dict())
    x = torch.randn(2, 16, 9, 7, requires_grad=True)
    x2 = x.detach().clone().requires_grad_(True)
    a(x).square().sum().backward()
    b(x2).square().sum().backward()
    assert torch.equal(a.weight.grad, b.weight.grad) and torch.equal(x.grad, x2.grad)


def test_flag_parses():
    for mode in ("dp", "ddp", "ddp_amp"):
        p = cli.build_parser(mode)
        assert p.parse_args([]).native_pointwise == "off"
        assert p.parse_args(["--native-pointwise", "on"]).native_pointwise == "on"
        assert p.parse_args(["--native-pointwise", "off"]).native_pointwise == "off"
        with pytest.raises(SystemExit):
            p.parse_args(["--native-pointwise", "auto"])


def _losses(tmp_path, flag):
    out = str(tmp_path / ("out_" + flag))
    args = ["dataparallel.py", "--outpath", out, "-a", "mobilenet_v2", "-b", "4", "--synthetic", "--synthetic-train-size",
            "8", "--synthetic-val-size", "4", "--image-size", "32", "--num-classes", "10", "-j", "0", "--epochs", "1",
            "--iters-per-epoch", "2", "--val-iters", "1", "--exist-policy", "delete", "-p", "1", "--seed", "3",
            "--no-tensorboard", "--native-pointwise", flag]
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
    assert "=> native pointwise: 34 conv(s) of mobilenet_v2 converted" in log_on
    assert "native pointwise" not in log_off
