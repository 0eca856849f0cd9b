"""7x7 depthwise-conv HIP kernels (csrc/kernels/dwconv7.hip), the ``DepthwiseConv7x7`` module and a converted
ConvNeXt-tiny training step on an MI355X.  References are plain ``F.conv2d`` / ``torch.nn.grad.conv2d_*`` on the CPU
from the rounded inputs.  Bounds are derived as in tests/test_depthwise_gpu.py, not tuned: per element

    |out - ref| <= u * |ref| + 4 * T * 2^-24 * A + s    forward / backward data against fp32; T = 49 (50 with bias),
                                                        A = the same op on |x|, |w|, |b|, u = 2^-8 / 2^-11,
                                                        s = one subnormal step of the dtype
    |dw - ref|  <= n * 2^-23 * A                        against fp64; n = N * H * W, A = conv2d_weight(|x|, |dy|)
    |db - ref|  <= n * 2^-23 * sum|dy|
"""
import copy

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
# (N, H, W, C).  The tiles are 8 rows x 32 columns x 8 channel vectors (W > 16), 8 x 16 x 16 (W <= 16) and 4 x 8 x 32
# (W <= 8): (1, 17, 33, 40), (2, 14, 14, 96) and (2, 7, 7, 16) give each a ragged last tile in every direction.
CASES = [
    (1, 1, 1, 8),      # only the centre tap is in bounds
    (2, 3, 5, 8),      # map smaller than the kernel, non-square
    (2, 7, 7, 16),     # every output touches padding; the 8-column tile
    (1, 17, 33, 40),   # more than one tile each way with ragged last tiles; 5 channel vectors
    (2, 14, 14, 96),   # the 16-column tile
    (1, 7, 7, 768),    # wide channels on a small map
    (3, 29, 31, 8),    # weight-gradient splits
]
_cache = {}


def _nchw(t):  # [N, H, W, C] -> logical NCHW (dense channels_last)
    return t.permute(0, 3, 1, 2)


def _oihw(w):  # taps-major [7, 7, C] -> [C, 1, 7, 7]
    return w.permute(2, 0, 1).unsqueeze(1)


def _refs(x, w, b, dy):
    """CPU references (NHWC / taps-major) in the precision of the arguments."""
    C = x.shape[3]
    xn, dyn, wo = _nchw(x), _nchw(dy), _oihw(w)
    y = F.conv2d(xn, wo, None, 1, 3, 1, C).permute(0, 2, 3, 1)
    dx = torch.nn.grad.conv2d_input(xn.shape, wo, dyn, 1, 3, 1, C).permute(0, 2, 3, 1)
    dw = torch.nn.grad.conv2d_weight(xn, wo.shape, dyn, 1, 3, 1, C)[:, 0].permute(1, 2, 0)
    return dict(y=y, yb=y + b, dx=dx, dw=dw, db=dy.sum((0, 1, 2)))


def _data(case, dtype):
    """Inputs on the GPU; references and their |.| counterparts on the CPU, computed once per (case, dtype)."""
    if (case, dtype) not in _cache:
        N, H, W, C = case
        g = torch.Generator().manual_seed(sum(case))
        t = [torch.randn(N, H, W, C, generator=g).to(dtype), (torch.randn(7, 7, C, generator=g) / 7).to(dtype),
             torch.randn(C, generator=g).to(dtype), torch.randn(N, H, W, C, generator=g).to(dtype)]
        d = dict(zip("xwbg", (v.to(DEV) for v in t)), n=N * H * W)
        for prec, keys in ((torch.float32, ("y", "yb", "dx")), (torch.float64, ("dw", "db"))):
            ref, mag = _refs(*(v.to(prec) for v in t)), _refs(*(v.to(prec).abs() for v in t))
            d.update({k: (ref[k], mag[k]) for k in keys})
        _cache[(case, dtype)] = d
    return _cache[(case, dtype)]


def _check16(out, ref_mag, T, what):
    ref, mag = ref_mag
    fi = torch.finfo(out.dtype)
    err = (out.float().cpu() - ref).abs()
    bound = U[out.dtype] * ref.abs() + 4 * T * 2.0 ** -24 * mag + fi.smallest_normal * fi.eps
    print(f"{what}: max err / bound {(err / bound).max().item():.3f}")
    assert out.shape == ref.shape and bool((err <= bound).all()), what


def _check32(got, ref_mag, n, what):
    ref, mag = ref_mag
    err, bound = (got.double().cpu() - ref).abs(), n * 2.0 ** -23 * mag
    print(f"{what}: max err / bound {(err / bound.clamp_min(1e-300)).max().item():.3e}")
    assert got.dtype == torch.float32 and got.shape == ref.shape and bool((err <= bound).all()), what


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("case", CASES)
def test_fwd(case, bias, dtype):
    from pytorch_distributed_template_amd.ops import depthwise7 as d7, native
    d = _data(case, dtype)
    b = d["b"] if bias else None
    y = d7.dwconv7_fwd(d["x"], d["w"], b)
    _check16(y, d["yb" if bias else "y"], 50 if bias else 49, f"fwd {case} bias={bias}")
    y2 = torch.empty_like(y)
    native.C.dwconv7_fwd(d["x"], d["w"], b, y2, *case)
    assert torch.equal(y, y2)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", CASES)
def test_dgrad(case, dtype):
    from pytorch_distributed_template_amd.ops import depthwise7 as d7, native
    d = _data(case, dtype)
    dx = d7.dwconv7_dgrad(d["g"], d["w"])
    _check16(dx, d["dx"], 49, f"dgrad {case}")
    dx2 = torch.empty_like(dx)
    native.C.dwconv7_dgrad(d["g"], d["w"], dx2, *case)
    assert torch.equal(dx, dx2)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("target", [None, 1, 4096])
@pytest.mark.parametrize("case", CASES)
def test_wgrad(case, target, dtype):
    from pytorch_distributed_template_amd.ops import depthwise7 as d7, native
    N, H, W, C = case
    d = _data(case, dtype)
    target = target or d7.WGRAD_TARGET_BLOCKS
    splits = native.C.dwconv7_wgrad_plan(N * H * W, C, target)[0]
    if case == (3, 29, 31, 8) and target in (1, 4096):
        assert splits == 1 if target == 1 else splits > 8
    dw, db = d7.dwconv7_wgrad(d["x"], d["g"], True, target)
    _check32(dw, d["dw"], d["n"], f"wgrad dw {case} splits={splits}")
    _check32(db, d["db"], d["n"], f"wgrad db {case} splits={splits}")
    ws = torch.empty((splits, 50, C), dtype=torch.float32, device=DEV)
    assert native.C.dwconv7_wgrad(d["x"], d["g"], ws, N, H, W, C, target) == splits
    dw2, db2 = d7.dwconv7_wgrad(d["x"], d["g"], True, target)
    assert torch.equal(dw, dw2) and torch.equal(db, db2) and d7.dwconv7_wgrad(d["x"], d["g"], False, target)[1] is None


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_hot_taps_are_exact(dtype):
    """Channel c carries the single weight 1.0 at tap c % 49: the forward is x shifted by that tap (zeros from the
    padding), the backward data the opposite shift, bit for bit."""
    from pytorch_distributed_template_amd.ops import depthwise7 as d7
    N, H, W, C = 2, 9, 11, 56
    x = torch.randn(N, H, W, C, generator=torch.Generator().manual_seed(7)).to(dtype)
    w = torch.zeros(49, C)
    w[torch.arange(C) % 49, torch.arange(C)] = 1.0
    xp = F.pad(x, (0, 0, 3, 3, 3, 3))
    fwd, bwd = torch.empty_like(x), torch.empty_like(x)
    for c in range(C):
        r, s = divmod(c % 49, 7)
        fwd[..., c] = xp[:, r:r + H, s:s + W, c]
        bwd[..., c] = xp[:, 6 - r:6 - r + H, 6 - s:6 - s + W, c]
    w16 = w.view(7, 7, C).to(dtype).to(DEV)
    assert torch.equal(d7.dwconv7_fwd(x.to(DEV), w16).cpu(), fwd)
    assert torch.equal(d7.dwconv7_dgrad(x.to(DEV), w16).cpu(), bwd)


@pytest.mark.parametrize("dtype", DTYPES)
def test_integers_are_exact(dtype):
    from pytorch_distributed_template_amd.ops import depthwise7 as d7
    g = torch.Generator().manual_seed(11)
    x, w, b, dy = (torch.randint(-3, 4, s, generator=g).double() for s in ((2, 9, 11, 16), (7, 7, 16), (16,), (2, 9, 11, 16)))
    ref = _refs(x, w, b, dy)
    assert ref["yb"].abs().max() < 256 and ref["dx"].abs().max() < 256  # exact in bf16
    x, w, b, dy = (v.to(dtype).to(DEV) for v in (x, w, b, dy))
    assert torch.equal(d7.dwconv7_fwd(x, w, b).double().cpu(), ref["yb"])
    assert torch.equal(d7.dwconv7_dgrad(dy, w).double().cpu(), ref["dx"])
    dw, db = d7.dwconv7_wgrad(x, dy, True)
    assert torch.equal(dw.double().cpu(), ref["dw"]) and torch.equal(db.double().cpu(), ref["db"])


def _counts():
    from pytorch_distributed_template_amd.ops import native
    c = native.C.dispatch_counts()
    return [c.get(k, 0) for k in ("dwconv7_fwd", "dwconv7_dgrad", "dwconv7_wgrad")]


def _delta(before):
    return [a - b for a, b in zip(_counts(), before)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("case", [(2, 7, 7, 16), (1, 17, 33, 40)])
def test_module_native_path(case, bias, dtype):
    from pytorch_distributed_template_amd.ops import depthwise7 as d7
    from pytorch_distributed_template_amd.optim.flat import FlatParams
    C = case[3]
    d = _data(case, dtype)
    model = nn.Sequential(nn.Conv2d(C, C, 7, padding=3, groups=C, bias=bias))
    assert d7.convert_depthwise7(model) == 1
    m = model[0]
    with torch.no_grad():  # masters = the case's (already 16-bit representable) weight and bias
        m.weight.copy_(_oihw(d["w"].float()))
        if bias:
            m.bias.copy_(d["b"].float())
    flat = FlatParams(model, torch.device(DEV), None)
    views = [p.grad for p in model.parameters()]
    y_op = d7.dwconv7_fwd(d["x"], d["w"], d["b"] if bias else None)
    gy = _nchw(d["g"]).contiguous()  # NCHW-contiguous: backward has to make it channels_last itself
    # a 16-bit input, then the same values as fp32 (ConvNeXt's residual stream), then one that needs no gradient
    for k, x in enumerate((_nchw(d["x"]), _nchw(d["x"]).float(), None), 1):
        x = _nchw(d["x"]) if x is None else x.detach().requires_grad_(True)
        assert x.is_contiguous(memory_format=torch.channels_last)
        before = _counts()
        with torch.autocast("cuda", dtype=dtype):
            y = m(x)
        assert _delta(before) == [1, 0, 0]  # no silent fallback
        assert y.dtype == dtype and y.is_contiguous(memory_format=torch.channels_last)
        assert torch.equal(y.permute(0, 2, 3, 1), y_op)
        y.backward(gy)
        assert _delta(before) == [1, int(x.requires_grad), 1]
        if k == 1:
            first = x.grad
            assert first.dtype == dtype
            _check16(first.permute(0, 2, 3, 1), d["dx"], 49, f"module dx {case}")
        elif k == 2:
            assert x.grad.dtype == torch.float32 and torch.equal(x.grad, first.float())  # the 16-bit dx, widened
        # the gradients land in the FlatParams views and accumulate there
        assert all(p.grad is v for p, v in zip(model.parameters(), views))
        _check32((flat.grad_flat(m.weight).view(C, 7, 7).permute(1, 2, 0) / k).contiguous(), d["dw"], d["n"],
                 f"module dw x{k} {case}")
        if bias:
            _check32(flat.grad_flat(m.bias) / k, d["db"], d["n"], f"module db x{k} {case}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_module_fallbacks(dtype):
    from pytorch_distributed_template_amd.ops import depthwise7 as d7
    torch.manual_seed(5)

    def same(x, c=32, k=7, stride=1):
        m = d7.DepthwiseConv7x7(c, c, k, stride=stride, padding=k // 2, groups=c).to(DEV)
        return torch.equal(m(x), F.conv2d(x, m.weight, m.bias, stride, k // 2, 1, c))

    cl = lambda c, dt: torch.randn(2, c, 9, 9, device=DEV).to(dt).contiguous(memory_format=torch.channels_last)
    before = _counts()
    assert same(cl(32, torch.float32))  # fp32 without autocast (the torch engine's validation)
    with torch.autocast("cuda", dtype=dtype):
        assert same(torch.randn(2, 32, 9, 9, device=DEV).to(dtype))  # NCHW input
        # non-qualifying convs on a channels_last 16-bit input
        assert same(cl(32, dtype), k=5) and same(cl(32, dtype), stride=2) and same(cl(60, dtype), c=60)
    assert _delta(before) == [0, 0, 0]


@pytest.mark.parametrize("dtype", DTYPES)
def test_convnext_tiny_train_step(dtype):
    """One torch-engine train step of ConvNeXt-tiny (no stochastic depth) with the 7x7 depthwise convs on the native
    kernels, against the same step in fp32 and judged against the stock autocast step (margins of
    tests/test_vgg_gpu.py).  No parameter of ConvNeXt has an analytically zero gradient: its LayerNorms normalise over
    the channels, which removes no per-channel constant."""
    from pytorch_distributed_template_amd.engine.torch_trainer import TorchTrainer
    from pytorch_distributed_template_amd.models import registry
    from pytorch_distributed_template_amd.ops import depthwise7 as d7
    torch.manual_seed(0)
    base = registry.create("convnext_tiny", stochastic_depth_prob=0.0)
    x, t = torch.randn(4, 3, 64, 64, device=DEV), torch.randint(0, 1000, (4,), device=DEV)
    m32, m16, mnat = copy.deepcopy(base), copy.deepcopy(base), copy.deepcopy(base)
    assert d7.convert_depthwise7(mnat) == 18
    rel = lambda a, b: ((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-12)).item()

    def run(model, dt):
        tr = TorchTrainer(model, DEV, dtype=dt)
        logits, _ = tr.train_step(x, t)
        torch.cuda.synchronize()
        return tr, logits, [p.grad.detach().clone() for p in model.parameters()]

    (_, l32, g32), (_, l16, g16) = run(m32, torch.float32), run(m16, dtype)
    before = _counts()
    tr, lnat, gnat = run(mnat, dtype)
    assert _delta(before) == [18, 18, 18]
    ours, theirs = rel(lnat, l32), rel(l16, l32)
    print(f"logits: native {ours:.4e}, autocast {theirs:.4e}")
    assert torch.isfinite(lnat).all() and ours < 1.5 * theirs + 0.02
    errs = [(n, rel(a, c), rel(b, c)) for (n, _), a, b, c in zip(base.named_parameters(), gnat, g16, g32)]
    print("gradient closest to the margin (name, native, autocast):", max(errs, key=lambda v: v[1] - 1.5 * v[2]))
    bad = [(n, round(eo, 4), round(et, 4)) for n, eo, et in errs if not eo < 1.5 * et + 0.01]
    assert not bad, bad[:8]
    before = _counts()  # validation runs in fp32 without autocast: every module falls back
    out, met = tr.eval_step(x, t)
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and torch.isfinite(met).all() and _delta(before) == [0, 0, 0]
