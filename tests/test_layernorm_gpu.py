"""LayerNorm HIP kernels (csrc/kernels/layernorm.hip), the ``NativeLayerNorm`` modules and a converted ConvNeXt-tiny
training step on an MI355X.  References are the plain fp64 formulas on the CPU from the rounded inputs.  Bounds are per
element, counted from the kernels' fp32 roundings (t = 2^-24), not tuned.  Per row, in fp64: mu, var, r = (var +
eps)^-1/2, xhat = (x - mu) * r, a = gamma * dy, and

    e_mu  = C * t * mean|x|                                  the sum of C terms, then the division
    e_d   = e_mu + t * |x - mu|                              x - mean as computed
    dvar  = 2 * e_mu * mean|x - mu| + (C + 4) * t * var      the shifted mean, then the sum of squares
    rho   = dvar / (2 * (var + eps)) + 4 * t                 relative error of rstd (add eps, divide, sqrt, reciprocal)
    e_xh  = r * e_d + rho * |xhat|                           xhat as computed
    |y - ref|      <= u * |ref| + |gamma| * r * e_d + rho * |gamma * xhat| + 3 * t * (|gamma * xhat| + |beta|) + s
    |dx - ref|     <= u * |ref| + r * (e_xh * |mean(a * xhat)| + |xhat| * mean(|a| * e_xh))
                      + (rho + (C + 16) * t) * r * (|a| + mean|a| + |xhat| * mean|a * xhat|) + s
    |dgamma - ref| <= rows * 2 * t * sum|dy * xhat| + sum(|dy| * e_xh)
    |dbeta - ref|  <= rows * 2 * t * sum|dy|

with u = 2^-8 (bf16), 2^-11 (fp16) or 2^-24 (an fp32 dx) for the one rounding of the output and s one subnormal step.
The bounds are worst cases over summation orders: a correct kernel passes by construction, and a ratio near 1 means
the count is wrong (largest ratios: profiles/layernorm_mi355x.md).
"""
import copy

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 2.0 ** -24}
T = 2.0 ** -24
EPS = 1e-6
# (rows, C, kind, beta, x dtypes: 16 = the 16-bit dtype, 32 = fp32)
CASES = [
    (1, 8, "randn", True, (16, 32)),       # one vector, L = 1
    (5, 96, "randn", False, (16, 32)),     # idle lanes (12 of L = 16); the rows do not fill a wave; no beta
    (67, 40, "randn", True, (16, 32)),     # masked vectors (5 of L = 8); ragged rows
    (130, 768, "randn", True, (16, 32)),   # NV = 2, several blocks
    (3, 2048, "randn", True, (16, 32)),    # the widest row: NV = 4, L = 64
    (1030, 24, "randn", True, (16, 32)),   # also with max_blocks = 1: the grid-stride loop, many partial rows
    (9, 384, "offset", True, (32,)),       # x = 1000 + randn in fp32: E[x^2] - mean^2 is wrong by tens of percent
    (4, 64, "const", True, (16, 32)),      # constant rows: var = 0, rstd = eps^-1/2, y ~ beta
    (530, 768, "randn", True, (16,)),      # 133 row groups on 160 blocks (27 idle): the two-stage sum of the partials
    (6, 1160, "randn", True, (16, 32)),    # NV = 3 with masked vectors (145 of 192)
]
PARAMS = [(c, xk) for c in CASES for xk in c[4]]
_cache = {}


def _data(case, dtype, xk):
    """Inputs on the GPU, fp64 references and bounds on the CPU, computed once per (case, dtype, x dtype)."""
    key = (case, dtype, xk)
    if key not in _cache:
        rows, C, kind, has_beta, _ = case
        gen = torch.Generator().manual_seed(rows + C)
        xdt = dtype if xk == 16 else torch.float32
        x = torch.randn(rows, C, generator=gen)
        if kind == "offset":
            x = x + 1000.0
        if kind == "const":
            x = torch.tensor([0.5, -3.0, 100.0, 1.25]).view(4, 1).expand(4, C).contiguous()
        x, dy = x.to(xdt), torch.randn(rows, C, generator=gen).to(dtype)
        g, b = 1 + 0.5 * torch.randn(C, generator=gen), (torch.randn(C, generator=gen) if has_beta else None)
        xd, gd, dyd, bd = x.double(), g.double(), dy.double(), (b.double() if has_beta else torch.zeros(C).double())
        m = lambda v: v.mean(1, keepdim=True)
        mu = m(xd)
        d = xd - mu
        var = m(d * d)
        r = (var + EPS).rsqrt()
        xh, a = d * r, gd * dyd
        e_mu = C * T * m(xd.abs())
        e_d = e_mu + T * d.abs()
        rho = (2 * e_mu * m(d.abs()) + (C + 4) * T * var) / (2 * (var + EPS)) + 4 * T
        e_xh = r * e_d + rho * xh.abs()
        ref = dict(y=xh * gd + bd, dx=r * (a - m(a) - xh * m(a * xh)), dg=(dyd * xh).sum(0), db=dyd.sum(0), mu=mu, r=r)
        bound = dict(
            y=gd.abs() * r * e_d + rho * (gd * xh).abs() + 3 * T * ((gd * xh).abs() + bd.abs()),
            dx=r * (e_xh * m(a * xh).abs() + xh.abs() * m(a.abs() * e_xh))
            + (rho + (C + 16) * T) * r * (a.abs() + m(a.abs()) + xh.abs() * m((a * xh).abs())),
            dg=rows * 2 * T * (dyd * xh).abs().sum(0) + (dyd.abs() * e_xh).sum(0), db=rows * 2 * T * dyd.abs().sum(0),
            mu=e_mu, r=rho * r)
        _cache[key] = dict(x=x.to(DEV), dy=dy.to(DEV), g=g.to(DEV), b=b.to(DEV) if has_beta else None, ref=ref,
                           bound=bound)
    return _cache[key]


def _check(got, d, k, what, rounded=True):
    ref, bound = d["ref"][k].reshape(got.shape), d["bound"][k].reshape(got.shape)
    if rounded:  # the one rounding of a stored activation
        fi = torch.finfo(got.dtype)
        bound = bound + U[got.dtype] * ref.abs() + fi.smallest_normal * fi.eps
    err = (got.double().cpu() - ref).abs()
    print(f"{what} {k}: max err / bound {(err / bound.clamp_min(1e-300)).max().item():.3e}")
    assert bool((err <= bound).all()), (what, k)


def _counts():
    from pytorch_distributed_template_amd.ops import native
    c = native.C.dispatch_counts()
    return [c.get(k, 0) for k in ("layernorm_fwd", "layernorm_bwd")]


def _delta(before):
    return [a - b for a, b in zip(_counts(), before)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case,xk", PARAMS)
def test_fwd_bwd(case, xk, dtype):
    from pytorch_distributed_template_amd.ops import layernorm as ln, native
    rows, C = case[:2]
    d = _data(case, dtype, xk)
    x, dy, g, b = d["x"], d["dy"], d["g"], d["b"]
    plans = {mb: ln.layernorm_plan(rows, C, mb) for mb in ((None, 1) if case[:2] == (1030, 24) else (None,))}
    if len(plans) == 2:
        assert plans[1][2] == 1 < plans[None][2] and plans[1][:2] == plans[None][:2]
    assert case[:2] != (1, 8) or plans[None][:2] == (1, 1)
    assert case[:2] != (3, 2048) or plans[None][:2] == (64, 4)
    assert case[:2] != (6, 1160) or plans[None][:2] == (64, 3)
    assert case[:2] != (530, 768) or plans[None][2] == 160
    for mb, plan in plans.items():
        what = f"{case[:3]} x{xk} plan={plan}"
        y, mean, rstd = ln.layernorm_fwd(x, g, b, EPS, dtype, mb)
        assert y.dtype == dtype and mean.dtype == rstd.dtype == torch.float32
        _check(y, d, "y", what)
        _check(mean, d, "mu", what, rounded=False)
        _check(rstd, d, "r", what, rounded=False)
        if case[2] == "const":
            assert torch.equal(mean, x[:, 0].float())  # the sums of these values are exact
        dx, dg, db = ln.layernorm_bwd(dy, x, mean, rstd, g, True, mb)
        assert dx.dtype == x.dtype and dg.dtype == db.dtype == torch.float32
        _check(dx, d, "dx", what)
        _check(dg, d, "dg", what, rounded=False)
        _check(db, d, "db", what, rounded=False)
        # bit-identical: twice through the ops, through the raw bindings, and dx without the gamma / beta sums
        again = ln.layernorm_fwd(x, g, b, EPS, dtype, mb) + ln.layernorm_bwd(dy, x, mean, rstd, g, True, mb)
        assert all(torch.equal(p, q) for p, q in zip(again, (y, mean, rstd, dx, dg, db)))
        mbi = mb or ln.MAX_BLOCKS
        y2, m2, r2, dx2 = torch.empty_like(y), torch.empty_like(mean), torch.empty_like(rstd), torch.empty_like(dx)
        native.C.layernorm_fwd(x, g, b, y2, m2, r2, rows, C, EPS, mbi)
        ws = torch.empty((plan[2], 2, C), dtype=torch.float32, device=DEV)
        assert tuple(native.C.layernorm_plan(rows, C, mbi)) == plan
        assert native.C.layernorm_bwd(dy, x, mean, rstd, g, dx2, ws, rows, C, mbi) == plan[2]
        assert torch.equal(y, y2) and torch.equal(mean, m2) and torch.equal(rstd, r2) and torch.equal(dx, dx2)
        _check(ws.double().sum(0)[0], d, "dg", what + " partials", rounded=False)
        dx3, none_g, none_b = ln.layernorm_bwd(dy, x, mean, rstd, g, False, mb)
        assert torch.equal(dx, dx3) and none_g is None and none_b is None


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", [CASES[2], CASES[3]])
def test_module_native_path(case, dtype):
    from pytorch_distributed_template_amd.ops import layernorm as ln
    from pytorch_distributed_template_amd.models.modern import LayerNorm2d
    from pytorch_distributed_template_amd.optim.flat import FlatParams
    rows, C = case[:2]
    d = _data(case, dtype, 16)
    model = nn.Sequential(nn.LayerNorm(C, eps=EPS), LayerNorm2d(C, eps=EPS))
    assert ln.convert_layernorm(model) == 2
    with torch.no_grad():
        for m in model:
            m.weight.copy_(d["g"])
            m.bias.copy_(d["b"])
    flat = FlatParams(model, torch.device(DEV), None)
    views = [p.grad for p in model.parameters()]
    y_op, mean, rstd = ln.layernorm_fwd(d["x"], d["g"], d["b"], EPS, dtype)
    dx_op = ln.layernorm_bwd(d["dy"], d["x"], mean, rstd, d["g"])[0]
    cl = lambda t: t.view(1, rows, 1, C).permute(0, 3, 1, 2)  # NCHW view of NHWC storage: dense channels_last
    k = 0
    for m, shape in ((model[0], lambda t: t.view(rows, C)), (model[1], cl)):
        for xin in (d["x"], d["x"].float()):  # a 16-bit input, then the same values as fp32
            k += 1
            x = shape(xin).detach().requires_grad_(True)
            before = _counts()
            with torch.autocast("cuda", dtype=dtype):
                y = m(x)
            assert _delta(before) == [1, 0] and y.dtype == dtype  # no silent fallback; the autocast dtype
            assert torch.equal(y.reshape(-1) if m is model[0] else y.permute(0, 2, 3, 1).reshape(-1), y_op.view(-1))
            y.backward(shape(d["dy"]))
            assert _delta(before) == [1, 1] and x.grad.dtype == xin.dtype
            gx = x.grad if m is model[0] else x.grad.permute(0, 2, 3, 1)
            if xin.dtype == dtype:
                assert torch.equal(gx.reshape(-1), dx_op.view(-1))
            else:
                _check(gx.reshape(rows, C), d, "dx", f"module fp32 dx {case[:2]}")
            # the gradients land in the FlatParams views and accumulate there
            assert all(p.grad is v for p, v in zip(model.parameters(), views))
            n = k if m is model[0] else k - 2
            _check(flat.grad_flat(m.weight) / n, d, "dg", f"module dgamma x{n} {case[:2]}", rounded=False)
            _check(flat.grad_flat(m.bias) / n, d, "db", f"module dbeta x{n} {case[:2]}", rounded=False)


@pytest.mark.parametrize("dtype", DTYPES)
def test_module_fallbacks(dtype):
    from pytorch_distributed_template_amd.ops import layernorm as ln
    torch.manual_seed(5)

    def same(x, c=64, **kw):
        m = ln.NativeLayerNorm(c, **kw).to(DEV)
        return torch.equal(m(x), F.layer_norm(x, (c,), m.weight, m.bias, m.eps))

    before = _counts()
    assert same(torch.randn(6, 64, device=DEV))  # no autocast (the torch engine's validation)
    with torch.autocast("cuda", dtype=dtype):
        assert same(torch.randn(6, 128, device=DEV).to(dtype)[:, ::2])  # strided
        assert same(torch.randn(6, 20, device=DEV).to(dtype), c=20)  # C % 8
        assert same(torch.randn(6, 64, device=DEV).to(dtype), elementwise_affine=False)
    assert _delta(before) == [0, 0]


@pytest.mark.parametrize("dtype", DTYPES)
def test_convnext_tiny_train_step(dtype):
    """One torch-engine train step of ConvNeXt-tiny (no stochastic depth) with its 23 LayerNorms on the native kernels,
    against the same step in fp32 and judged against the stock autocast step (the comparison and margins of
    tests/test_dwconv7_gpu.py)."""
    from pytorch_distributed_template_amd.engine.torch_trainer import TorchTrainer
    from pytorch_distributed_template_amd.models import registry
    from pytorch_distributed_template_amd.ops import layernorm as ln
    torch.manual_seed(0)
    base = registry.create("convnext_tiny", stochastic_depth_prob=0.0)
    x, t = torch.randn(4, 3, 64, 64, device=DEV), torch.randint(0, 1000, (4,), device=DEV)
    m32, m16, mnat = copy.deepcopy(base), copy.deepcopy(base), copy.deepcopy(base)
    assert ln.convert_layernorm(mnat) == 23
    rel = lambda a, b: ((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-12)).item()

    def run(model, dt):
        tr = TorchTrainer(model, DEV, dtype=dt)
        logits, _ = tr.train_step(x, t)
        torch.cuda.synchronize()
        return tr, logits, [p.grad.detach().clone() for p in model.parameters()]

    (_, l32, g32), (_, l16, g16) = run(m32, torch.float32), run(m16, dtype)
    before = _counts()
    tr, lnat, gnat = run(mnat, dtype)
    assert _delta(before) == [23, 23]
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
    assert torch.isfinite(out).all() and torch.isfinite(met).all() and _delta(before) == [0, 0]
