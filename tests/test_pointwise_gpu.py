"""Pointwise-conv HIP kernels (csrc/kernels/pwconv.hip), the ``PointwiseConv2d`` module and a converted MobileNetV2
training step on an MI355X.

Cases, operands, references and the two layers of judgement are tests/_pointwise_cases.py's (proven on the CPU by
tests/test_pointwise_cpu.py): layer A (integers) bit for bit, layer B (reals) within tests/_numerics.py's
``assert_conv`` bound with n the reduction length -- no margin on either.
"""
import copy

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import _numerics as nm
import _pointwise_cases as pc

pytestmark = pytest.mark.gpu

DEV = "cuda"
KERNELS = ("pwconv_fwd", "pwconv_dgrad", "pwconv_wgrad")
_ids = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v).split(".")[-1]
ALL = pytest.mark.parametrize("g,dtype,layer", [(g, dt, la) for g in pc.GEOMS for dt in pc.DTYPES for la in pc.LAYERS],
                              ids=_ids)


def _C():
    from pytorch_distributed_template_amd.ops import native
    return native.C


def _pw():
    from pytorch_distributed_template_amd.ops import pointwise
    return pointwise


def _counts():
    c = _C().dispatch_counts()
    return {k: c.get(k, 0) for k in KERNELS}


def _delta(before):
    after = _counts()
    return {k: after[k] - before[k] for k in before}


def _d(**kw):
    return {k: kw.get(k.split("_")[1], 0) for k in KERNELS}


def _relnorm(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-12)).item()


def _nchw(t):  # [N, H, W, C] -> logical NCHW (dense channels_last)
    return t.permute(0, 3, 1, 2)


# ------------------------------------------------------------------------------------------ the functional ops
@ALL
def test_pwconv_fwd(g, dtype, layer):
    pw = _pw()
    d = pc.case("fwd", g, dtype, layer)
    x, w = d["x"].to(DEV), d["w"].to(DEV)
    y = pw.pwconv_fwd(x, w)
    assert y.dtype == dtype and y.is_contiguous()
    pc.judge(y.cpu(), d, dtype, layer, f"fwd {g}", "pwconv_fwd")
    assert torch.equal(y, pw.pwconv_fwd(x, w))  # run to run


@ALL
def test_pwconv_dgrad(g, dtype, layer):
    pw = _pw()
    d = pc.case("dgrad", g, dtype, layer)
    dy, w = d["dy"].to(DEV), d["w"].to(DEV)
    dx = pw.pwconv_dgrad(dy, w)
    assert dx.dtype == dtype and dx.is_contiguous()
    pc.judge(dx.cpu(), d, dtype, layer, f"dgrad {g}", "pwconv_dgrad")
    assert torch.equal(dx, pw.pwconv_dgrad(dy, w))
    assert torch.equal(dx, pw.pwconv_dgrad(dy, w, w.t().contiguous()))  # the caller's own transpose


@ALL
def test_pwconv_wgrad(g, dtype, layer):
    pw = _pw()
    N, H, W, C, K = g
    d = pc.case("wgrad", g, dtype, layer)
    x, dy = d["x"].to(DEV), d["dy"].to(DEV)
    for tb in pc.WGRAD_TARGETS:
        kw = {} if tb is None else {"target_blocks": tb}
        dw = pw.pwconv_wgrad(x, dy, **kw)
        assert dw.is_contiguous()
        pc.judge_dw(dw.cpu(), d, layer, f"wgrad {g} target_blocks={tb}")
        assert torch.equal(dw, pw.pwconv_wgrad(x, dy, **kw))
    if g == pc.WGRAD_PLAN_GEOM:
        s1 = pw.pwconv_wgrad_plan(pc.rows(g), C, K, 1)[0]
        s2 = pw.pwconv_wgrad_plan(pc.rows(g), C, K, 4096)[0]
        print("plan splits:", s1, s2)
        assert s1 == 1 and s2 > 8


@pytest.mark.parametrize("g", pc.TINY_GEOMS, ids=_ids)
def test_pwconv_wgrad_subnormal_dy(g):
    """fp16 dY that is subnormal (what the unscaled fp16 torch-engine step hands the kernel): within ``assert_conv``'s bound
    over the nominal magnitudes (tests/_numerics.py), for every split count, bit for bit the same on a second run."""
    pw = _pw()
    d = pc.case("wgrad", g, torch.float16, "tiny")
    x, dy = d["x"].to(DEV), d["dy"].to(DEV)
    assert float((dy.float().abs() < 2.0 ** -14).float().mean()) > 0.999 and float((dy != 0).float().mean()) > 0.99
    for tb in pc.WGRAD_TARGETS:
        kw = {} if tb is None else {"target_blocks": tb}
        dw = pw.pwconv_wgrad(x, dy, **kw)
        pc.judge_dw(dw.cpu(), d, "tiny", f"tiny wgrad {g} target_blocks={tb}", "pwconv_wgrad_tiny")
        assert torch.equal(dw, pw.pwconv_wgrad(x, dy, **kw))


def test_plan_and_size_predicate():
    """The plan covers every pixel with whole reduction steps, and the size predicate is the contract."""
    C_ = _C()
    for M, C, K, tb in ((1, 8, 8, 1024), (297, 16, 96, 1024), (3136, 32, 192, 4096), (5017600, 16, 96, 1024),
                        (19600, 960, 320, 1024)):
        splits, pps, ct, kt = C_.pwconv_wgrad_plan(M, C, K, tb)
        assert pps % 128 == 0 and (splits - 1) * pps < M <= splits * pps
        assert ct == -(-C // 64) and kt == -(-K // 64)
    assert C_.pwconv_fits(1, 8, 8) and C_.pwconv_fits(400 * 112 * 112, 16, 96) and C_.pwconv_fits(1 << 30, 2048, 2048)
    for M, C, K in ((0, 8, 8), ((1 << 30) + 1, 8, 8), (16, 4, 8), (16, 8, 12), (16, 2056, 8), (16, 8, 2056)):
        assert not C_.pwconv_fits(M, C, K)
    x = torch.zeros(16, 12, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError):  # a launcher refuses what the predicate refuses
        C_.pwconv_fwd(x, torch.zeros(8, 12, dtype=torch.bfloat16, device=DEV),
                      torch.zeros(16, 8, dtype=torch.bfloat16, device=DEV), 16, 12, 8)


# ------------------------------------------------------------------------------------------ isolation
PAD = 1024  # elements around every view: a multiple of 8, the views stay 16-byte aligned
CANARY = 7.0


def _inside(t, fill):
    """``t``'s values as a contiguous view in the middle of a larger buffer filled with ``fill``."""
    buf = torch.full((t.numel() + 2 * PAD,), fill, dtype=t.dtype, device=DEV)
    view = buf[PAD:PAD + t.numel()].view(t.shape)
    view.copy_(t)
    return buf, view


def _canaries_intact(buf, n):
    return bool((buf[:PAD] == CANARY).all() and (buf[PAD + n:] == CANARY).all())


@pytest.mark.parametrize("dtype", pc.DTYPES, ids=_ids)
@pytest.mark.parametrize("g", pc.ISOLATION_GEOMS, ids=_ids)
@pytest.mark.parametrize("kind", ["fwd", "dgrad"])
def test_isolation(kind, g, dtype):
    """Operands and output in the middle of larger buffers (NaN around the inputs, a canary around the output) and one
    whole input pixel NaN: only that pixel's output row is non-finite, every other element keeps its bound, nothing
    is written outside the output."""
    N, H, W, C, K = g
    M = pc.rows(g)
    d = pc.case(kind, g, dtype, "real")
    a = d["x" if kind == "fwd" else "dy"].reshape(M, -1).clone()
    bad = M // 2 + 1
    a[bad] = float("nan")
    nout = K if kind == "fwd" else C
    _, av = _inside(a, float("nan"))
    obuf, ov = _inside(torch.full((M, nout), CANARY, dtype=dtype), CANARY)
    if kind == "fwd":
        _, wv = _inside(d["w"], float("nan"))
        _C().pwconv_fwd(av, wv, ov, M, C, K)
    else:
        _, wv = _inside(d["w"].t().contiguous(), float("nan"))
        _C().pwconv_dgrad(av, wv, ov, M, C, K)
    torch.cuda.synchronize()
    out = ov.cpu()
    assert _canaries_intact(obuf, M * nout)
    assert torch.isnan(out[bad]).all()
    keep = torch.arange(M) != bad
    assert torch.isfinite(out[keep]).all()
    ref, mag = d["ref"].reshape(M, nout)[keep], d["mag"].reshape(M, nout)[keep]
    nm.assert_conv(out[keep], ref, mag, d["n"], dtype, f"isolation {kind} {g}", "pwconv_" + kind)


@pytest.mark.parametrize("dtype", pc.DTYPES, ids=_ids)
@pytest.mark.parametrize("g", pc.ISOLATION_GEOMS, ids=_ids)
def test_isolation_wgrad(g, dtype):
    N, H, W, C, K = g
    M = pc.rows(g)
    d = pc.case("wgrad", g, dtype, "real")
    _, xv = _inside(d["x"].reshape(M, C), float("nan"))
    _, dv = _inside(d["dy"].reshape(M, K), float("nan"))
    splits = _C().pwconv_wgrad_plan(M, C, K, 4096)[0]
    wbuf, wsv = _inside(torch.full((splits, K, C), CANARY, dtype=torch.float32), CANARY)
    assert _C().pwconv_wgrad(xv, dv, wsv, M, C, K, 4096) == splits
    dbuf, dwv = _inside(torch.full((K, C), CANARY, dtype=torch.float32), CANARY)
    _C().wgrad_reduce(wsv, splits, K, C, C, K * C, dwv, C, 1.0, False)
    torch.cuda.synchronize()
    assert _canaries_intact(wbuf, splits * K * C) and _canaries_intact(dbuf, K * C)
    pc.judge_dw(dwv.cpu().contiguous(), d, "real", f"isolation wgrad {g}")


# ------------------------------------------------------------------------------------------ the module
@pytest.mark.parametrize("dtype", pc.DTYPES, ids=_ids)
@pytest.mark.parametrize("g", [(3, 9, 11, 16, 96), (2, 7, 9, 96, 24), (5, 13, 13, 40, 200)], ids=_ids)
def test_module_native_path(g, dtype):
    pw = _pw()
    N, H, W, C, K = g
    f, b, wg = (pc.case(k, g, dtype, "real") for k in ("fwd", "dgrad", "wgrad"))
    m = pw.PointwiseConv2d(C, K, 1, bias=False).to(DEV)
    x_nhwc = f["x"].to(DEV)
    with torch.no_grad():  # master weight = the case's (already 16-bit representable) weight as [K, C, 1, 1] fp32
        m.weight.copy_(f["w"].float().view(K, C, 1, 1))
    x = _nchw(x_nhwc).detach().requires_grad_(True)  # NHWC storage seen as NCHW: dense channels_last
    assert x.is_contiguous(memory_format=torch.channels_last)
    y_op = pw.pwconv_fwd(x_nhwc, f["w"].to(DEV))
    before = _counts()
    with torch.autocast("cuda", dtype=dtype):
        y = m(x)
    assert _delta(before) == _d(fwd=1)  # no silent fallback
    assert y.dtype == dtype and y.shape == (N, K, H, W)
    assert y.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(y.permute(0, 2, 3, 1), y_op)
    pc.judge(y.permute(0, 2, 3, 1).cpu(), f, dtype, "real", f"module y {g}", "pwconv_fwd")

    # the backward pass on operands of its own: the module with the dgrad case's weight and the wgrad case's x / dy
    with torch.no_grad():
        m.weight.copy_(b["w"].float().view(K, C, 1, 1))
    x = _nchw(wg["x"].to(DEV)).detach().requires_grad_(True)
    gy = _nchw(b["dy"].to(DEV)).contiguous()  # NCHW-contiguous: backward has to make it channels_last itself
    assert not gy.is_contiguous(memory_format=torch.channels_last) or K == 1
    before = _counts()
    with torch.autocast("cuda", dtype=dtype):
        y = m(x)
    assert _delta(before) == _d(fwd=1)
    y.backward(gy)
    assert _delta(before) == _d(fwd=1, dgrad=1, wgrad=1)
    assert x.grad.dtype == dtype and x.grad.shape == x.shape
    pc.judge(x.grad.permute(0, 2, 3, 1).cpu(), b, dtype, "real", f"module dx {g}", "pwconv_dgrad")
    gw = m.weight.grad
    assert gw.dtype == torch.float32 and gw.shape == m.weight.shape == (K, C, 1, 1)
    # dw of (the wgrad case's x, the dgrad case's dy): its own fp64 reference
    ref, mag = nm.conv_wgrad_ref(wg["x"], b["dy"], 1, 1, 1, 0)
    dd = dict(ref=ref.reshape(K, C), mag=mag.reshape(K, C), n=pc.rows(g))
    pc.judge_dw(gw.view(K, C).cpu(), dd, "real", f"module dw {g}")
    # input without gradient: no backward-data launch
    m.weight.grad = None
    before = _counts()
    with torch.autocast("cuda", dtype=dtype):
        y = m(_nchw(wg["x"].to(DEV)))
    y.backward(gy)
    assert _delta(before) == _d(fwd=1, wgrad=1)
    assert torch.equal(m.weight.grad, gw)


def test_module_gradient_accumulates_into_flat_views():
    """The fp32 [K, C, 1, 1] gradient lands in (and accumulates into) the ``.grad`` views of FlatParams."""
    from pytorch_distributed_template_amd.optim.flat import FlatParams
    pw = _pw()
    g, dtype = (3, 9, 11, 16, 96), torch.bfloat16
    N, H, W, C, K = g
    d = pc.case("wgrad", g, dtype, "real")
    model = nn.Sequential(nn.Conv2d(C, K, 1, bias=False))
    assert pw.convert_pointwise(model) == 1
    flat = FlatParams(model, torch.device(DEV), None)
    view = model[0].weight.grad
    x, gy = _nchw(d["x"].to(DEV)), _nchw(d["dy"].to(DEV))
    for k in (1, 2):
        with torch.autocast("cuda", dtype=dtype):
            y = model(x)
        y.backward(gy)
        assert model[0].weight.grad is view  # still the flat view
        got = flat.grad_flat(model[0].weight).view(K, C) / k
        pc.judge_dw(got.cpu().contiguous(), d, "real", f"flat accumulation x{k}")


@pytest.mark.parametrize("dtype", pc.DTYPES, ids=_ids)
def test_module_fallbacks(dtype):
    pw = _pw()
    torch.manual_seed(5)
    C, K = 32, 64
    m = pw.PointwiseConv2d(C, K, 1, bias=False).to(DEV)
    x32 = torch.randn(2, C, 9, 9, device=DEV).contiguous(memory_format=torch.channels_last)
    x16 = torch.randn(2, C, 9, 9, device=DEV).to(dtype)  # NCHW-contiguous
    assert not x16.is_contiguous(memory_format=torch.channels_last)
    before = _counts()
    # fp32 without autocast (the torch engine's validation)
    assert torch.equal(m(x32), F.conv2d(x32, m.weight))
    with torch.autocast("cuda", dtype=dtype):
        # NCHW 16-bit input
        assert torch.equal(m(x16), F.conv2d(x16, m.weight))
        # non-qualifying convs on a channels_last 16-bit input: biased, stride 2, 58 channels
        for cin, kw in ((32, dict(bias=True)), (32, dict(stride=2, bias=False)), (58, dict(bias=False))):
            mm = pw.PointwiseConv2d(cin, K, 1, **kw).to(DEV)
            xx = torch.randn(2, cin, 9, 9, device=DEV).to(dtype).contiguous(memory_format=torch.channels_last)
            assert torch.equal(mm(xx), F.conv2d(xx, mm.weight, mm.bias, mm.stride))
    assert _delta(before) == _d()


# ------------------------------------------------------------------------------------------ MobileNetV2
_mnv2 = {}


def _mobilenet(dtype):
    """The shared arms of the train-step tests: the fp32 step once, the stock autocast step once per dtype."""
    from pytorch_distributed_template_amd.engine.torch_trainer import TorchTrainer
    from pytorch_distributed_template_amd.models import registry
    if "base" not in _mnv2:
        torch.manual_seed(0)
        base = registry.create("mobilenet_v2", dropout=0.0)
        x = torch.randn(8, 3, 64, 64, device=DEV)
        t = torch.randint(0, 1000, (8,), device=DEV)

        def run(model, dt):
            tr = TorchTrainer(model, DEV, dtype=dt)
            logits, met = tr.train_step(x, t)
            torch.cuda.synchronize()
            return tr, logits, [p.grad.detach().clone() for _, p in model.named_parameters()]
        _mnv2.update(base=base, x=x, t=t, run=run)
        _, _mnv2["l32"], _mnv2["g32"] = run(copy.deepcopy(base), torch.float32)
    if dtype not in _mnv2:
        _, l16, g16 = _mnv2["run"](copy.deepcopy(_mnv2["base"]), dtype)
        _mnv2[dtype] = (l16, g16)
    return _mnv2


@pytest.mark.parametrize("dtype", pc.DTYPES, ids=_ids)
def test_mobilenet_v2_train_step(dtype):
    """One torch-engine train step of MobileNetV2 (dropout 0) with only ``convert_pointwise`` applied, against the same
    step in fp32 and judged against the stock autocast step exactly as
    tests/test_depthwise_gpu.py::test_mobilenet_v2_train_step does (margins 1.5x + 0.02 for the logits, 1.5x + 0.01 for
    every gradient; the 17 analytically-zero projection-BN biases measured against the gradient norm of the same
    BatchNorm's scale)."""
    pw = _pw()
    r = _mobilenet(dtype)
    base, x, t, l32, g32 = r["base"], r["x"], r["t"], r["l32"], r["g32"]
    l16, g16 = r[dtype]
    mnat = copy.deepcopy(base)
    assert pw.convert_pointwise(mnat) == 34
    names = [n for n, _ in base.named_parameters()]
    assert [n for n, _ in mnat.named_parameters()] == names
    before = _counts()
    tr, lnat, gnat = r["run"](mnat, dtype)
    assert _delta(before) == _d(fwd=34, dgrad=34, wgrad=34)  # no silent fallback
    ours, theirs = _relnorm(lnat, l32), _relnorm(l16, l32)
    print(f"logits: native {ours:.4e}, autocast {theirs:.4e}")
    assert torch.isfinite(lnat).all()
    assert ours < 1.5 * theirs + 0.02
    zero_of = {n + ".conv." + str(len(m.conv) - 1) + ".bias": n + ".conv." + str(len(m.conv) - 1) + ".weight"
               for n, m in base.named_modules() if isinstance(getattr(m, "conv", None), nn.Sequential)}
    assert len(zero_of) == 17 and set(zero_of) <= set(names)
    gi = {n: i for i, n in enumerate(names)}
    bad = []
    for n, a, b, c in zip(names, gnat, g16, g32):
        if n in zero_of:
            scale = g32[gi[zero_of[n]]].norm()
            assert c.norm() < 1e-3 * scale, (n, c.norm().item(), scale.item())  # zero up to fp32 rounding
            eo, et = (a.norm() / scale).item(), (b.norm() / scale).item()
        else:
            eo, et = _relnorm(a, c), _relnorm(b, c)
        if not eo < 1.5 * et + 0.01:
            bad.append((n, round(eo, 4), round(et, 4)))
    worst = max(((n, _relnorm(a, c), _relnorm(b, c)) for n, a, b, c in zip(names, gnat, g16, g32) if n not in zero_of),
                key=lambda v: v[1] - 1.5 * v[2])
    print("gradient closest to the margin (name, native, autocast):", worst)
    assert not bad, bad[:8]
    npw = 0
    for m in mnat.modules():
        if isinstance(m, pw.PointwiseConv2d):
            g = tr.flat.grad_flat(m.weight)
            assert torch.isfinite(g).all() and (g != 0).any()
            npw += 1
    assert npw == 34
    # validation runs in fp32 without autocast: every module falls back
    before = _counts()
    out, met = tr.eval_step(x, t)
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and torch.isfinite(met).all()
    assert _delta(before) == _d()


@pytest.mark.parametrize("dtype", pc.DTYPES, ids=_ids)
def test_mobilenet_v2_all_three_conversions(dtype):
    """Pointwise, depthwise and BatchNorm+activation conversions together: every native path runs and the step is
    finite (no accuracy margin on this arm: profiles/bnact_mi355x.md records that the comparison is noise-limited)."""
    from pytorch_distributed_template_amd.ops import bnact, depthwise
    pw = _pw()
    r = _mobilenet(dtype)
    m = copy.deepcopy(r["base"])
    assert pw.convert_pointwise(m) == 34 and depthwise.convert_depthwise(m) == 17
    assert bnact.convert_bnact(m) == (52, 35)
    names = ("dwconv_fwd", "dwconv_dgrad", "dwconv_wgrad", "bnact_stats", "bnact_fwd", "bnact_bwd_reduce", "bnact_bwd_apply")
    c0 = _C().dispatch_counts()
    before = _counts()
    tr, logits, grads = r["run"](m, dtype)
    c1 = _C().dispatch_counts()
    assert _delta(before) == _d(fwd=34, dgrad=34, wgrad=34)
    assert {k: c1.get(k, 0) - c0.get(k, 0) for k in names} == {k: (17 if k.startswith("dw") else 52) for k in names}
    assert torch.isfinite(logits).all() and all(torch.isfinite(g).all() for g in grads)
