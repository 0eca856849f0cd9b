"""First-conv HIP kernels (csrc/kernels/stem3x3.hip), the ``StemConv2d`` module and a converted MobileNetV2 training
step on an MI355X.

Cases, operands, references and the layers of judgement are tests/_stem3x3_cases.py's (proven on the CPU by
tests/test_stem3x3_cpu.py): layer A (integers) bit for bit, layer B (reals) and the rounding layer (an fp32 image that
needs the in-kernel rounding) within tests/_numerics.py's ``assert_conv`` bound with n the reduction length -- no margin
on any of them.
"""
import copy

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import _conv_cases as cc
import _numerics as nm
import _stem3x3_cases as sc

pytestmark = pytest.mark.gpu

DEV = "cuda"
KERNELS = ("stem3x3_fwd", "stem3x3_wgrad")
_ids = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v).split(".")[-1]
ALL = pytest.mark.parametrize("g,dtype,layer", [(g, dt, la) for g in sc.GEOMS for dt in sc.DTYPES for la in sc.LAYERS],
                              ids=_ids)
NAN = float("nan")


def _C():
    from pytorch_distributed_template_amd.ops import native
    return native.C


def _st():
    from pytorch_distributed_template_amd.ops import stemconv
    return stemconv


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


def _run_fwd(x, w, g):
    """The forward launcher into an output pre-filled with NaN."""
    N, H, W, K = g
    P, Q = sc.out_hw(g)
    y = torch.full((N, P, Q, K), NAN, dtype=w.dtype, device=DEV)
    _C().stem3x3_fwd(x, w, y, N, H, W, K)
    return y


def _run_wgrad(x, dy, g, tb):
    """Launcher and reduction into a workspace and a gradient pre-filled with NaN."""
    N, H, W, K = g
    C_ = _C()
    splits = C_.stem3x3_wgrad_plan(sc.rows(g), K, tb)[0]
    ws = torch.full((splits, K, 32), NAN, dtype=torch.float32, device=DEV)
    assert C_.stem3x3_wgrad(x, dy, ws, N, H, W, K, tb) == splits
    assert not torch.isnan(ws).any() and (ws[:, :, 27:] == 0).all()  # every slab wholly written, slots 27..31 zero
    dw = torch.full((K, 3, 3, 3), NAN, dtype=torch.float32, device=DEV)
    C_.wgrad_reduce(ws, splits, K, 27, 32, K * 32, dw, 27, 1.0, False)
    return dw


# ------------------------------------------------------------------------------------------ the functional ops
@ALL
def test_stem3x3_fwd(g, dtype, layer):
    st = _st()
    d = sc.case("fwd", g, dtype, layer)
    x, w = d["x32"].to(DEV), d["w"].to(DEV)
    y = _run_fwd(x, w, g)
    sc.judge(y.cpu(), d, dtype, layer, f"fwd {g}", "stem3x3_fwd")
    y2 = st.stem3x3_fwd(x, w)  # the functional op, run to run
    assert y2.dtype == dtype and y2.is_contiguous() and torch.equal(y, y2)


@ALL
def test_stem3x3_wgrad(g, dtype, layer):
    st = _st()
    N, H, W, K = g
    d = sc.case("wgrad", g, dtype, layer)
    x, dy = d["x32"].to(DEV), d["dy"].to(DEV)
    for tb in sc.WGRAD_TARGETS:
        kw = {} if tb is None else {"target_blocks": tb}
        dw = _run_wgrad(x, dy, g, st.WGRAD_TARGET_BLOCKS if tb is None else tb)
        sc.judge_dw(dw.cpu(), d, layer, f"wgrad {g} target_blocks={tb}")
        dw2 = st.stem3x3_wgrad(x, dy, **kw)
        assert dw2.is_contiguous() and torch.equal(dw, dw2)
    if g == sc.WGRAD_PLAN_GEOM:
        s1 = st.stem3x3_wgrad_plan(sc.rows(g), K, 1)[0]
        s2 = st.stem3x3_wgrad_plan(sc.rows(g), K, 4096)[0]
        print("plan splits:", s1, s2)
        assert s1 == 1 and s2 > 8


@pytest.mark.parametrize("g", sc.TINY_GEOMS, ids=_ids)
def test_stem3x3_wgrad_subnormal_dy(g):
    """fp16 dY that is subnormal (what the unscaled fp16 torch-engine step hands the kernel): within ``assert_conv``'s bound
    over the nominal magnitudes (tests/_numerics.py), for every split count, and the op agrees with the launcher."""
    st = _st()
    d = sc.case("wgrad", g, torch.float16, "tiny")
    x, dy = d["x32"].to(DEV), d["dy"].to(DEV)
    assert float((dy.float().abs() < 2.0 ** -14).float().mean()) > 0.999 and float((dy != 0).float().mean()) > 0.99
    for tb in sc.WGRAD_TARGETS:
        kw = {} if tb is None else {"target_blocks": tb}
        dw = _run_wgrad(x, dy, g, st.WGRAD_TARGET_BLOCKS if tb is None else tb)
        sc.judge_dw(dw.cpu(), d, "tiny", f"tiny wgrad {g} target_blocks={tb}", "stem3x3_wgrad_tiny")
        assert torch.equal(dw, st.stem3x3_wgrad(x, dy, **kw))


def test_plan_and_size_predicate():
    """The plan covers every pixel with whole reduction steps, and the size predicate is the contract."""
    C_ = _C()
    for M, K, tb in ((1, 8, 1024), (105, 32, 1024), (3136, 32, 4096), (3136, 32, 1), (400 * 112 * 112, 32, 1024),
                     (1 << 30, 64, 1024), (1 << 30, 8, 1), ((1 << 30) - 77, 16, 4096)):
        splits, pps = C_.stem3x3_wgrad_plan(M, K, tb)
        assert pps % 128 == 0 and splits >= 1 and (splits - 1) * pps < M <= splits * pps
    fits = lambda N, H, W, K: C_.stem3x3_fits(N, H, W, K)
    assert fits(1, 1, 1, 8) and fits(400, 224, 224, 32) and fits(350000, 32, 32, 8) and fits(1, 1, 2, 64)
    assert fits(1 << 30, 1, 2, 8) and fits(1 << 20, 63, 64, 16)      # N * P * Q = 2^30
    assert not fits((1 << 30) + 1, 1, 2, 8) and not fits((1 << 20) + 1, 63, 64, 16)  # one over
    for K in (4, 12, 72, 0, 60):
        assert not fits(2, 8, 8, K)
    for N, H, W in ((0, 8, 8), (1, 0, 8), (1, 8, 0)):
        assert not fits(N, H, W, 8)
    # one image must stay below 2^31 bytes: 13377^2 * 12 B is just below, 13378^2 * 12 B and 2^14 x 2^15 x 12 B above
    assert fits(1, 13377, 13377, 8) and not fits(1, 13378, 13378, 8) and not fits(1, 1 << 14, 1 << 15, 8)
    x = torch.zeros(2, 8, 8, 3, device=DEV)
    with pytest.raises(RuntimeError):  # a launcher refuses what the predicate refuses
        C_.stem3x3_fwd(x, torch.zeros(12, 3, 3, 3, dtype=torch.bfloat16, device=DEV),
                       torch.zeros(2, 4, 4, 12, dtype=torch.bfloat16, device=DEV), 2, 8, 8, 12)
    with pytest.raises(RuntimeError):
        C_.stem3x3_wgrad(x, torch.zeros(2, 4, 4, 72, dtype=torch.bfloat16, device=DEV),
                         torch.zeros(1, 72, 32, device=DEV), 2, 8, 8, 72, 1024)
    with pytest.raises(RuntimeError):  # operands that do not match the geometry
        C_.stem3x3_fwd(x, torch.zeros(8, 3, 3, 3, dtype=torch.bfloat16, device=DEV),
                       torch.zeros(2, 4, 4, 8, dtype=torch.bfloat16, device=DEV), 2, 8, 9, 8)
    with pytest.raises(RuntimeError):  # a 16-bit image is not this kernel's input
        C_.stem3x3_fwd(x.bfloat16(), torch.zeros(8, 3, 3, 3, dtype=torch.bfloat16, device=DEV),
                       torch.zeros(2, 4, 4, 8, dtype=torch.bfloat16, device=DEV), 2, 8, 8, 8)
    with pytest.raises(RuntimeError):  # a workspace smaller than the plan
        C_.stem3x3_wgrad(torch.zeros(4, 56, 56, 3, device=DEV), torch.zeros(4, 28, 28, 32, dtype=torch.bfloat16, device=DEV),
                         torch.zeros(2, 32, 32, device=DEV), 4, 56, 56, 32, 4096)


# ------------------------------------------------------------------------------------------ isolation
PAD = 1024  # elements around every view: a multiple of 8, the 16-bit and fp32 views stay 16-byte aligned
CANARY = 7.0


def _inside(t, fill):
    """``t``'s values as a contiguous view in the middle of a larger buffer filled with ``fill``."""
    buf = torch.full((t.numel() + 2 * PAD,), fill, dtype=t.dtype, device=DEV)
    view = buf[PAD:PAD + t.numel()].view(t.shape)
    view.copy_(t)
    return buf, view


def _canaries_intact(buf, n):
    return bool((buf[:PAD] == CANARY).all() and (buf[PAD + n:] == CANARY).all())


POISON = 32768.0  # finite in both 16-bit types: a product with a zero dY is an exact zero


def _poisoned(x, side, value):
    """The image with the elements that lie right next to a padding position in memory set to ``value``.  "before": the
    last column of every row and the last row of every image, which is where a left / top padding read (column -1,
    row -1) lands when it is not replaced by zero; "after": the first column and the first row (column W, row H)."""
    x = x.clone()
    i = -1 if side == "before" else 0
    x[:, :, i] = value
    x[:, i] = value
    return x


def _windows_holding(mask):
    """[N, P, Q] bool: the output pixels whose 3x3 window holds a marked element of the [N, H, W, 3] image."""
    return nm.conv_fwd_ref(mask.double(), torch.ones(1, 3, 3, 3, dtype=torch.float64), 2, 1)[0][..., 0] > 0


@pytest.mark.parametrize("dtype", sc.DTYPES, ids=_ids)
@pytest.mark.parametrize("g", sc.ISOLATION_GEOMS, ids=_ids)
def test_isolation_fwd(g, dtype):
    """The image as a view inside a NaN-filled buffer (a read outside the image poisons the output), the output as a
    view inside a canary-filled buffer.  Padding must come out as zeros, not as neighbours' memory: with the elements
    next to the padding positions NaN, exactly the outputs whose window holds such an element are NaN and every other
    one keeps its bound."""
    N, H, W, K = g
    P, Q = sc.out_hw(g)
    d = sc.case("fwd", g, dtype, "real")
    _, xv = _inside(d["x32"], NAN)
    _, wv = _inside(d["w"], NAN)
    ybuf, yv = _inside(torch.full((N, P, Q, K), CANARY, dtype=dtype), CANARY)
    _C().stem3x3_fwd(xv, wv, yv, N, H, W, K)
    torch.cuda.synchronize()
    assert _canaries_intact(ybuf, N * P * Q * K)
    sc.judge(yv.cpu(), d, dtype, "real", f"isolation fwd {g}", "stem3x3_fwd")
    for side in ("before", "after"):
        x = _poisoned(d["x32"], side, NAN)
        _, xv = _inside(x, NAN)
        y = _run_fwd(xv, wv, g).cpu()
        hit = _windows_holding(torch.isnan(x))
        assert hit.any() and (~hit).any()
        assert torch.isnan(y[hit]).all() and torch.isfinite(y[~hit]).all(), side
        nm.assert_conv(y[~hit], d["ref"][~hit], d["mag"][~hit], 27, dtype, f"isolation fwd {g}: {side}", "stem3x3_fwd")


@pytest.mark.parametrize("dtype", sc.DTYPES, ids=_ids)
@pytest.mark.parametrize("g", sc.ISOLATION_GEOMS, ids=_ids)
def test_isolation_wgrad(g, dtype):
    """Image and dY inside NaN-filled buffers, workspace and gradient inside canary-filled ones.  Padding: the elements
    next to the padding positions hold a large finite value and dY is zero on every window that holds one of them, so
    the value can reach dw only through a read that padding should have replaced."""
    N, H, W, K = g
    d = sc.case("wgrad", g, dtype, "real")
    _, xv = _inside(d["x32"], NAN)
    _, dv = _inside(d["dy"], NAN)
    splits = _C().stem3x3_wgrad_plan(sc.rows(g), K, 4096)[0]
    wbuf, wsv = _inside(torch.full((splits, K, 32), CANARY, dtype=torch.float32), CANARY)
    assert _C().stem3x3_wgrad(xv, dv, wsv, N, H, W, K, 4096) == splits
    dbuf, dwv = _inside(torch.full((K, 3, 3, 3), CANARY, dtype=torch.float32), CANARY)
    _C().wgrad_reduce(wsv, splits, K, 27, 32, K * 32, dwv, 27, 1.0, False)
    torch.cuda.synchronize()
    assert _canaries_intact(wbuf, splits * K * 32) and _canaries_intact(dbuf, K * 27)
    assert (wsv[:, :, 27:] == 0).all()
    sc.judge_dw(dwv.cpu().contiguous(), d, "real", f"isolation wgrad {g}")
    for side in ("before", "after"):
        x = _poisoned(d["x32"], side, POISON)
        hit = _windows_holding(x == POISON)
        assert hit.any() and (~hit).any()
        dy = d["dy"].clone()
        dy[hit] = 0
        _, xv = _inside(x, NAN)
        dw = _run_wgrad(xv, dy.to(DEV), g, 4096).cpu()
        ref, mag = nm.conv_wgrad_ref(x.to(dtype), dy, 3, 3, 2, 1)
        nm.assert_conv(dw, ref, mag, sc.rows(g), torch.float32, f"isolation wgrad {g}: {side}", "stem3x3_wgrad")


# ------------------------------------------------------------------------------------------ a far image
def test_far_image():
    """350,000 images of 32 x 32: the image tensor (4.3 GB) passes 2^32 bytes, so image bases must be 64-bit.  All zeros
    but a small random case in the first two and the last two images: their outputs equal the op's result on those 4
    images alone bit for bit, an image in the middle gives zeros.  dw, with dy zero outside the same images, is judged
    against the fp64 reference of the four images with n = their 4 * 256 pixels: every other product is an exact zero,
    and adding zeros (within a slab or in wgrad_reduce) rounds nothing."""
    st = _st()
    free = torch.cuda.mem_get_info()[0]
    if free < 12e9:
        pytest.skip(f"needs 12 GB of free GPU memory, {free / 1e9:.1f} GB are free")
    N, H, W, K, dtype = 350000, 32, 32, 8, torch.bfloat16
    assert N * H * W * 3 * 4 > 2 ** 32 and st.fits(N, H, W, K)
    g4 = (4, H, W, K)
    f, b = sc.case("fwd", g4, dtype, "round"), sc.case("wgrad", g4, dtype, "round")
    sel = [0, 1, N - 2, N - 1]
    w = f["w"].to(DEV)
    x = torch.zeros(N, H, W, 3, device=DEV)
    x[sel] = f["x32"].to(DEV)
    y4 = st.stem3x3_fwd(f["x32"].to(DEV), w)
    sc.judge(y4.cpu(), f, dtype, "round", "far image: the 4-image case", None)
    y = st.stem3x3_fwd(x, w)
    assert torch.equal(y[sel], y4)
    assert (y[N // 2] == 0).all() and (y[2] == 0).all() and (y[N - 3] == 0).all()
    del y
    x[sel] = b["x32"].to(DEV)
    dy = torch.zeros(N, 16, 16, K, dtype=dtype, device=DEV)
    dy[sel] = b["dy"].to(DEV)
    dw = st.stem3x3_wgrad(x, dy)
    sc.judge_dw(dw.cpu(), b, "round", "far image dw")
    assert torch.equal(dw, st.stem3x3_wgrad(x, dy))
    del x, dy
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------ the module
@pytest.mark.parametrize("dtype", sc.DTYPES, ids=_ids)
@pytest.mark.parametrize("g", [(2, 9, 7, 24), (3, 10, 13, 32), (5, 17, 15, 48)], ids=_ids)
def test_module_native_path(g, dtype):
    st = _st()
    N, H, W, K = g
    P, Q = sc.out_hw(g)
    f, b = sc.case("fwd", g, dtype, "round"), sc.case("wgrad", g, dtype, "real")
    m = st.StemConv2d(3, K, 3, stride=2, padding=1, bias=False).to(DEV)
    with torch.no_grad():  # master weight = the case's (already 16-bit representable) KRSC weight as fp32 (K, C, R, S)
        m.weight.copy_(f["w"].float().permute(0, 3, 1, 2))
    x = _nchw(f["x32"].to(DEV))  # NHWC storage seen as NCHW: dense channels_last
    assert x.is_contiguous(memory_format=torch.channels_last) and not x.requires_grad
    y_op = st.stem3x3_fwd(f["x32"].to(DEV), f["w"].to(DEV))
    before = _counts()
    with torch.autocast("cuda", dtype=dtype):
        y = m(x)
    assert _delta(before) == _d(fwd=1)  # no silent fallback
    assert y.dtype == dtype and y.shape == (N, K, P, Q)
    assert y.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(y.permute(0, 2, 3, 1), y_op)
    sc.judge(y.permute(0, 2, 3, 1).cpu(), f, dtype, "round", f"module y {g}", "stem3x3_fwd")

    # the backward pass on the wgrad case's operands, with an NCHW-contiguous gy: backward makes it NHWC itself
    x = _nchw(b["x32"].to(DEV))
    gy = _nchw(b["dy"].to(DEV)).contiguous()
    assert not gy.is_contiguous(memory_format=torch.channels_last)
    before = _counts()
    with torch.autocast("cuda", dtype=dtype):
        y = m(x)
    assert _delta(before) == _d(fwd=1)
    y.backward(gy)
    assert _delta(before) == _d(fwd=1, wgrad=1)
    gw = m.weight.grad
    assert gw.dtype == torch.float32 and gw.shape == m.weight.shape == (K, 3, 3, 3)
    sc.judge_dw(gw.permute(0, 2, 3, 1).contiguous().cpu(), b, "real", f"module dw {g}")  # (K, C, R, S) -> KRSC


def test_module_gradient_accumulates_into_flat_views():
    """The fp32 [K, 3, 3, 3] gradient lands in (and accumulates into) the ``.grad`` views of FlatParams."""
    from pytorch_distributed_template_amd.optim.flat import FlatParams
    st = _st()
    g, dtype = (3, 10, 13, 32), torch.bfloat16
    N, H, W, K = g
    d = sc.case("wgrad", g, dtype, "real")
    model = nn.Sequential(nn.Conv2d(3, K, 3, stride=2, padding=1, bias=False))
    assert st.convert_stem(model) == 1
    flat = FlatParams(model, torch.device(DEV), None)
    view = model[0].weight.grad
    x, gy = _nchw(d["x32"].to(DEV)), _nchw(d["dy"].to(DEV))
    for k in (1, 2):
        before = _counts()
        with torch.autocast("cuda", dtype=dtype):
            y = model(x)
        y.backward(gy)
        assert _delta(before) == _d(fwd=1, wgrad=1)
        assert model[0].weight.grad is view  # still the flat view
        got = flat.grad_flat(model[0].weight).view(K, 3, 3, 3) / k  # conv weights are stored KRSC in the flat buffers
        sc.judge_dw(got.cpu().contiguous(), d, "real", f"flat accumulation x{k}")


@pytest.mark.parametrize("dtype", sc.DTYPES, ids=_ids)
def test_module_fallbacks(dtype):
    st = _st()
    torch.manual_seed(5)
    K = 32
    conv = lambda mm, xx: F.conv2d(xx, mm.weight, mm.bias, mm.stride, mm.padding)
    m = st.StemConv2d(3, K, 3, stride=2, padding=1, bias=False).to(DEV)
    xcl = torch.randn(2, 3, 9, 9, device=DEV).contiguous(memory_format=torch.channels_last)
    xnchw = torch.randn(2, 3, 9, 9, device=DEV)
    assert not xnchw.is_contiguous(memory_format=torch.channels_last)
    before = _counts()
    # fp32 without autocast (the torch engine's validation, --precision fp32)
    assert torch.equal(m(xcl), conv(m, xcl))
    with torch.autocast("cuda", dtype=dtype):
        # NCHW-contiguous input
        assert torch.equal(m(xnchw), conv(m, xnchw))
        # 16-bit input
        x16 = xcl.to(dtype)
        assert x16.is_contiguous(memory_format=torch.channels_last)
        assert torch.equal(m(x16), conv(m, x16))
        # an input that requires grad: its gradient exists
        xg = xcl.clone().requires_grad_(True)
        xr = xcl.clone().requires_grad_(True)
        y, yr = m(xg), conv(m, xr)
        assert torch.equal(y, yr)
        y.float().square().sum().backward()
        yr.float().square().sum().backward()
        assert xg.grad is not None and xg.grad.shape == xg.shape and torch.isfinite(xg.grad).all()
        assert (xg.grad != 0).any()
        # non-qualifying instances on the kernels' own kind of input: biased, stride 1, K = 12
        for k, kw in ((K, dict(stride=2, bias=True)), (K, dict(stride=1, bias=False)), (12, dict(stride=2, bias=False))):
            mm = st.StemConv2d(3, k, 3, padding=1, **kw).to(DEV)
            assert torch.equal(mm(xcl), conv(mm, xcl))
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


@pytest.mark.parametrize("dtype", sc.DTYPES, ids=_ids)
def test_mobilenet_v2_train_step(dtype):
    """One torch-engine train step of MobileNetV2 (dropout 0) at 8 x 64 x 64 with only ``convert_stem`` applied, against
    the same step in fp32 and judged against the stock autocast step exactly as
    tests/test_pointwise_gpu.py::test_mobilenet_v2_train_step judges its arm (margins 1.5x + 0.02 for the logits,
    1.5x + 0.01 for every gradient; the 17 analytically-zero projection-BN biases measured against the gradient norm of
    the same BatchNorm's scale)."""
    st = _st()
    r = _mobilenet(dtype)
    base, x, t, l32, g32 = r["base"], r["x"], r["t"], r["l32"], r["g32"]
    l16, g16 = r[dtype]
    mnat = copy.deepcopy(base)
    assert st.convert_stem(mnat) == 1
    names = [n for n, _ in base.named_parameters()]
    assert [n for n, _ in mnat.named_parameters()] == names
    before = _counts()
    tr, lnat, gnat = r["run"](mnat, dtype)
    assert _delta(before) == _d(fwd=1, wgrad=1)  # no silent fallback
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
    nst = 0
    for m in mnat.modules():
        if isinstance(m, st.StemConv2d):
            g = tr.flat.grad_flat(m.weight)
            assert torch.isfinite(g).all() and (g != 0).any()
            nst += 1
    assert nst == 1
    # validation runs in fp32 without autocast: the module falls back
    before = _counts()
    out, met = tr.eval_step(x, t)
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and torch.isfinite(met).all()
    assert _delta(before) == _d()


@pytest.mark.parametrize("dtype", sc.DTYPES, ids=_ids)
def test_mobilenet_v2_all_four_conversions(dtype):
    """Stem, pointwise, depthwise and BatchNorm+activation conversions together: every native path runs and the step
    is finite (no accuracy margin on this arm: profiles/bnact_mi355x.md records that the comparison is noise-limited;
    the per-layer verdict on this configuration is tests/test_torch_audit_gpu.py)."""
    from pytorch_distributed_template_amd.ops import bnact, depthwise, pointwise
    st = _st()
    r = _mobilenet(dtype)
    m = copy.deepcopy(r["base"])
    assert st.convert_stem(m) == 1 and pointwise.convert_pointwise(m) == 34 and depthwise.convert_depthwise(m) == 17
    assert bnact.convert_bnact(m) == (52, 35)
    want = {"pwconv_fwd": 34, "pwconv_dgrad": 34, "pwconv_wgrad": 34, "dwconv_fwd": 17, "dwconv_dgrad": 17,
            "dwconv_wgrad": 17, "bnact_stats": 52, "bnact_fwd": 52, "bnact_bwd_reduce": 52, "bnact_bwd_apply": 52}
    c0 = _C().dispatch_counts()
    before = _counts()
    tr, logits, grads = r["run"](m, dtype)
    c1 = _C().dispatch_counts()
    assert _delta(before) == _d(fwd=1, wgrad=1)
    assert {k: c1.get(k, 0) - c0.get(k, 0) for k in want} == want
    assert torch.isfinite(logits).all() and all(torch.isfinite(g).all() for g in grads)
