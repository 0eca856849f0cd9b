"""First-conv (3x3, stride 2, 3 channels) cases, module conversion and the ``--native-stem`` flag without a GPU.

* the cases of tests/_stem3x3_cases.py are proven before any kernel runs: the layer-A condition holds on every
  reference, and a torch emulation of a correct kernel (the image rounded to the dtype, an fp32 unfold + matmul rounded
  once; the weight gradient summed split by split) passes every geometry, dtype and layer;
* mutations of that emulation -- a dropped tap, the window shifted by one, the bottom row / right column of an
  odd-sided image read as real data, channels reversed, r and s swapped in dw, the image truncated instead of rounded,
  a NaN in reduction slot 27, a weight gradient without its last split, a neighbouring channel's weights -- each fail
  the same check on at least one case (and on every case where the mutation changes a value);
* which convs of the registry models qualify, that conversion keeps parameters / state dict / CPU results, the flag,
  and a CPU run with the flag on equals one with it off (the module falls back to ``F.conv2d`` there).
"""
import copy
import os
import re
import subprocess
import sys

import pytest
import torch
import torch.nn as nn

import _numerics as nm
import _stem3x3_cases as sc
from pytorch_distributed_template_amd import cli
from pytorch_distributed_template_amd.models import registry
from pytorch_distributed_template_amd.ops.stemconv import StemConv2d, convert_stem, qualifies

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CONVERTED = ["mobilenet_v2", "mobilenet_v3_large", "mobilenet_v3_small", "mnasnet1_0", "efficientnet_b0",
             "efficientnet_b3", "efficientnet_b7", "shufflenet_v2_x1_0"]
NOT_CONVERTED = ["resnet18", "vgg11", "squeezenet1_1", "inception_v3", "densenet121"]

GD = [(g, dt) for g in sc.GEOMS for dt in sc.DTYPES]
_ids = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v).split(".")[-1]


# ------------------------------------------------------------------------------ the cases, on references alone
@pytest.mark.parametrize("g,dtype", GD, ids=_ids)
def test_layer_a_conditions(g, dtype):
    """Integer outputs are exactly representable in the 16-bit type; every partial sum of the weight gradient is an
    integer far below 2**24."""
    assert nm.int_case_conditions(sc.case("fwd", g, dtype, "int")["ref"], dtype, g[3])[0] == 0.0
    assert sc.case("wgrad", g, dtype, "int")["mag"].max().item() < 2.0 ** 20


@pytest.mark.parametrize("g,dtype", GD, ids=_ids)
def test_round_layer_is_not_representable(g, dtype):
    """The rounding layer's image really needs the rounding: most of its values change when cast to the dtype."""
    for kind in ("fwd", "wgrad"):
        d = sc.case(kind, g, dtype, "round")
        assert (d["x"].float() != d["x32"]).float().mean().item() > 0.9


@pytest.mark.parametrize("layer", sc.LAYERS)
@pytest.mark.parametrize("g,dtype", GD, ids=_ids)
def test_emulation_passes(g, dtype, layer):
    d = sc.case("fwd", g, dtype, layer)
    sc.judge(sc.emul_fwd(d["x32"], d["w"], dtype), d, dtype, layer, f"fwd {g}", None)
    d = sc.case("wgrad", g, dtype, layer)
    for pps in (128, 1 << 20):
        sc.judge_dw(sc.emul_wgrad(d["x32"], d["dy"], dtype, pps), d, layer, f"wgrad {g}", None)


# ------------------------------------------------------------------------------ mutations must fail the same check
def _fwd_rejected(d, dtype, layer, name, **mut):
    with pytest.raises(AssertionError):
        sc.judge(sc.emul_fwd(d["x32"], d["w"], dtype, **mut), d, dtype, layer, name, None)


def _dw_rejected(d, dtype, layer, name, pps=128, **mut):
    with pytest.raises(AssertionError):
        sc.judge_dw(sc.emul_wgrad(d["x32"], d["dy"], dtype, pps, **mut), d, layer, name, None)


@pytest.mark.parametrize("layer", ["int", "real"])
@pytest.mark.parametrize("g,dtype", GD, ids=_ids)
def test_structural_mutations_fail(g, dtype, layer):
    N, H, W, K = g
    f, b = sc.case("fwd", g, dtype, layer), sc.case("wgrad", g, dtype, layer)
    # a tap that meets image data at some output pixel of this geometry: the centre always does
    for tap in [(1, 1)] + ([(0, 0)] if H > 2 and W > 2 else []) + ([(2, 2)] if H > 1 and W > 1 else []):
        _fwd_rejected(f, dtype, layer, f"dropped tap {tap}", drop_tap=tap)
        _dw_rejected(b, dtype, layer, f"dropped tap {tap}", drop_tap=tap)
    _fwd_rejected(f, dtype, layer, "window shifted by one", pad0=True)
    _dw_rejected(b, dtype, layer, "window shifted by one", pad0=True)
    _fwd_rejected(f, dtype, layer, "channels reversed", reverse_c=True)
    _dw_rejected(b, dtype, layer, "channels reversed", reverse_c=True)
    _fwd_rejected(f, dtype, layer, "NaN in slot 27", slot27=float("nan"))
    _fwd_rejected(f, dtype, layer, "neighbouring channel's weights", neighbour_w=True)
    if H > 1 and W > 1:  # a 1 x Q map has one row of taps only: r and s cannot be told apart by their values
        _dw_rejected(b, dtype, layer, "r and s swapped", swap_rs=True)
    # the padding below / right of an odd-sided image read as real data (even sides never read it)
    if H % 2 == 1 and H > 1:
        _fwd_rejected(f, dtype, layer, "bottom padding row reads data", real_bottom=True)
        _dw_rejected(b, dtype, layer, "bottom padding row reads data", real_bottom=True)
    if W % 2 == 1 and W > 1:
        _fwd_rejected(f, dtype, layer, "right padding column reads data", real_right=True)
        _dw_rejected(b, dtype, layer, "right padding column reads data", real_right=True)


@pytest.mark.parametrize("g,dtype", GD, ids=_ids)
def test_even_sides_never_read_bottom_right_padding(g, dtype):
    """The counterpart: on an even side that mutation changes nothing, so the odd-sided geometries own it."""
    N, H, W, K = g
    d = sc.case("fwd", g, dtype, "real")
    good = sc.emul_fwd(d["x32"], d["w"], dtype)
    if H % 2 == 0:
        assert torch.equal(good, sc.emul_fwd(d["x32"], d["w"], dtype, real_bottom=True))
    if W % 2 == 0:
        assert torch.equal(good, sc.emul_fwd(d["x32"], d["w"], dtype, real_right=True))


@pytest.mark.parametrize("g,dtype", GD, ids=_ids)
def test_truncated_image_fails_rounding_layer(g, dtype):
    """Truncation of the image instead of round-to-nearest-even: visible in the layer whose image needs rounding."""
    _fwd_rejected(sc.case("fwd", g, dtype, "round"), dtype, "round", "truncated image", truncate=True)


@pytest.mark.parametrize("dtype", sc.DTYPES, ids=_ids)
def test_truncated_image_fails_a_weight_gradient(dtype):
    """The weight gradient's bound grows with n * mag while the error of truncation grows like sqrt(n): the short
    reductions own this mutation (the forward pass, n = 27, sees it on every geometry)."""
    rejected = []
    for g in sc.GEOMS:
        d = sc.case("wgrad", g, dtype, "round")
        try:
            sc.judge_dw(sc.emul_wgrad(d["x32"], d["dy"], dtype, 128, truncate=True), d, "round", "truncated image", None)
        except AssertionError:
            rejected.append(g)
    assert rejected


@pytest.mark.parametrize("g", sc.TINY_GEOMS, ids=_ids)
def test_tiny_layer_emulation_passes_and_mutations_fail(g):
    """fp16 weight gradient with subnormal dY (the ``real`` operand times 2**-16), judged over the nominal magnitudes: the
    emulation stays inside the bound; a missing split, a dropped centre tap and R / S swapped leave it."""
    dt = torch.float16
    d = sc.case("wgrad", g, dt, "tiny")
    a = d["dy"].float().abs()
    # subnormal and nonzero: all but the |dy| >= 4 and the |dy| < 2**-9 of a normal sample
    assert float((a < nm.FP16_MIN_NORMAL).float().mean()) > 0.999 and float((a > 0).float().mean()) > 0.99
    assert torch.equal(d["x32"], sc.case("wgrad", g, dt, "real")["x32"])
    plain = nm.conv_wgrad_ref(d["x"], d["dy"], 3, 3, 2, 1)[1]
    assert bool((d["mag"] >= plain).all()) and bool((d["mag"] > plain).any())
    for pps in (32, 1 << 20):
        sc.judge_dw(sc.emul_wgrad(d["x32"], d["dy"], dt, pps), d, "tiny", f"tiny wgrad {g}", None)
    for name, mut in (("missing split", dict(drop_last_split=True)), ("dropped tap", dict(drop_tap=(1, 1))),
                      ("R and S swapped", dict(swap_rs=True))):
        with pytest.raises(AssertionError):
            sc.judge_dw(sc.emul_wgrad(d["x32"], d["dy"], dt, 32, **mut), d, "tiny", name, None)


@pytest.mark.parametrize("layer", sc.LAYERS)
@pytest.mark.parametrize("g,dtype", GD, ids=_ids)
def test_wgrad_missing_split_fails(g, dtype, layer):
    d = sc.case("wgrad", g, dtype, layer)
    if sc.rows(g) > 128:
        _dw_rejected(d, dtype, layer, "missing split", drop_last_split=True)
    else:  # a single split: dropping it leaves zeros
        _dw_rejected(d, dtype, layer, "missing split", pps=1 << 20, drop_last_split=True)


# ------------------------------------------------------------------------------ module conversion
def test_qualifying_predicate():
    assert qualifies(nn.Conv2d(3, 32, 3, stride=2, padding=1, bias=False))
    for k in (8, 16, 24, 40, 48, 56, 64):
        assert qualifies(nn.Conv2d(3, k, 3, stride=2, padding=1, bias=False))
    for bad in (nn.Conv2d(3, 32, 3, stride=2, padding=1, bias=True),
                nn.Conv2d(3, 32, 3, stride=1, padding=1, bias=False),
                nn.Conv2d(3, 32, 3, stride=2, padding=0, bias=False),   # inception_v3's first conv
                nn.Conv2d(3, 12, 3, stride=2, padding=1, bias=False),
                nn.Conv2d(3, 72, 3, stride=2, padding=1, bias=False),
                nn.Conv2d(4, 32, 3, stride=2, padding=1, bias=False),
                nn.Conv2d(3, 32, 5, stride=2, padding=1, bias=False),
                nn.Conv2d(3, 32, 3, stride=2, padding=1, dilation=2, bias=False),
                nn.Conv2d(3, 33, 3, stride=2, padding=1, groups=3, bias=False),
                nn.Conv2d(3, 24, 3, stride=2, padding=1, groups=3, bias=False),
                nn.Conv2d(3, 32, (3, 1), stride=2, padding=1, bias=False),
                nn.Conv2d(3, 32, 3, stride=(2, 1), padding=1, bias=False)):
        assert not qualifies(bad), bad


@pytest.mark.parametrize("arch", CONVERTED)
def test_convert_counts_one(arch):
    model = registry.create(arch)
    names = [n for n, _ in model.named_parameters()]
    keys = list(model.state_dict().keys())
    assert convert_stem(model) == 1
    assert sum(isinstance(m, StemConv2d) for m in model.modules()) == 1
    assert [n for n, _ in model.named_parameters()] == names and list(model.state_dict().keys()) == keys
    assert convert_stem(model) == 0  # idempotent


@pytest.mark.parametrize("arch", NOT_CONVERTED)
def test_convert_counts_zero(arch):
    model = registry.create(arch)
    assert convert_stem(model) == 0
    assert not any(isinstance(m, StemConv2d) for m in model.modules())


def test_conversion_keeps_state_and_results():
    torch.manual_seed(0)
    model = registry.create("mobilenet_v2").eval()
    ref = copy.deepcopy(model)
    before = dict(model.state_dict())
    params = dict(model.named_parameters())
    hits = [n for n, m in model.named_modules() if isinstance(m, nn.Conv2d) and qualifies(m)]
    flags = {n: m.training for n, m in model.named_modules()}
    assert convert_stem(model) == 1 == len(hits)
    after = model.state_dict()
    assert list(after.keys()) == list(before.keys())
    assert all(after[k] is before[k] or torch.equal(after[k], before[k]) for k in before)
    mods = dict(model.named_modules())
    assert type(mods[hits[0]]) is StemConv2d
    assert mods[hits[0]].weight is params[hits[0] + ".weight"]  # the very same Parameter object
    assert [n for n, _ in model.named_parameters()] == list(params)
    assert {n: m.training for n, m in model.named_modules()} == flags
    x = torch.randn(2, 3, 32, 32)
    with torch.no_grad():
        assert torch.equal(model(x), ref(x))  # CPU: the module falls back to F.conv2d
    ref.load_state_dict(model.state_dict())
    model.load_state_dict(ref.state_dict())


def test_four_converters_in_two_orders():
    from pytorch_distributed_template_amd.ops.bnact import convert_bnact
    from pytorch_distributed_template_amd.ops.depthwise import convert_depthwise
    from pytorch_distributed_template_amd.ops.pointwise import convert_pointwise
    base = registry.create("mobilenet_v2")
    conv = {"pointwise": convert_pointwise, "depthwise": convert_depthwise, "bnact": convert_bnact, "stem": convert_stem}
    want = {"pointwise": 34, "depthwise": 17, "bnact": (52, 35), "stem": 1}
    classes = []
    for order in (("stem", "pointwise", "depthwise", "bnact"), ("bnact", "depthwise", "pointwise", "stem")):
        m = copy.deepcopy(base)
        assert {k: conv[k](m) for k in order} == want, order
        classes.append([(n, type(mod).__name__) for n, mod in m.named_modules()])
    assert classes[0] == classes[1]
    assert sum(c == "StemConv2d" for _, c in classes[0]) == 1


def test_module_constructor_and_cpu_gradients():
    torch.manual_seed(1)
    a = StemConv2d(3, 24, 3, stride=2, padding=1, bias=False)
    b = nn.Conv2d(3, 24, 3, stride=2, padding=1, bias=False)
    assert list(a.state_dict()) == list(b.state_dict()) and a.weight.shape == b.weight.shape == (24, 3, 3, 3)
    b.load_state_dict(a.state_dict())
    x = torch.randn(2, 3, 9, 7, requires_grad=True)
    x2 = x.detach().clone().requires_grad_(True)
    ya, yb = a(x), b(x2)
    assert torch.equal(ya, yb)
    ya.square().sum().backward()
    yb.square().sum().backward()
    assert torch.equal(a.weight.grad, b.weight.grad) and torch.equal(x.grad, x2.grad)
    with torch.autocast("cpu", dtype=torch.bfloat16):  # CPU autocast is not the kernels' case either
        assert torch.equal(a(x.detach()), b(x.detach()))


def test_flag_parses():
    for mode in ("dp", "ddp", "ddp_amp"):
        p = cli.build_parser(mode)
        assert p.parse_args([]).native_stem == "off"
        assert p.parse_args(["--native-stem", "on"]).native_stem == "on"
        assert p.parse_args(["--native-stem", "off"]).native_stem == "off"
        with pytest.raises(SystemExit):
            p.parse_args(["--native-stem", "auto"])


def _losses(tmp_path, flag):
    out = str(tmp_path / ("out_" + flag))
    args = ["dataparallel.py", "--outpath", out, "-a", "mobilenet_v2", "-b", "4", "--synthetic", "--synthetic-train-size",
            "8", "--synthetic-val-size", "4", "--image-size", "32", "--num-classes", "10", "-j", "0", "--epochs", "1",
            "--iters-per-epoch", "2", "--val-iters", "1", "--exist-policy", "delete", "-p", "1", "--seed", "3",
            "--no-tensorboard", "--native-stem", flag]
    env = dict(os.environ, PYTHONUNBUFFERED="1", OMP_NUM_THREADS="2", HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable] + args, cwd=ROOT, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    log = open(os.path.join(out + "_mobilenet_v2", "experiment.log")).read()
    return log, re.findall(r"Train epoch: \[0/1\]\[\d+/\d+\]\tlr=\S+\tce_loss=(\S+)\ttop1_acc=(\S+)", log)


def test_cpu_run_with_flag_on_equals_off(tmp_path):
    """Two iterations of mobilenet_v2 on CPU through the runner: the converted module falls back to F.conv2d, so the
    loss lines are those of the unconverted run."""
    log_on, on = _losses(tmp_path, "on")
    log_off, off = _losses(tmp_path, "off")
    assert len(off) == 2 and on == off, (on, off)
    assert "=> native stem: 1 conv(s) of mobilenet_v2 converted" in log_on
    assert "native stem" not in log_off
