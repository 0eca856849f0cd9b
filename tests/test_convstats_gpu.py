"""The pointwise conv's BatchNorm-statistics epilogue (``pwconv_fwd_stats``, csrc/kernels/pwconv.hip), the conv ->
BatchNorm hand-over of the converted modules (ops/convstats.py) and a MobileNetV2 step with all five conversions, on an
MI355X.

The kernel is judged on every geometry of tests/_pointwise_cases.py, both dtypes, both layers, from NaN-filled buffers:

* ``y`` is the plain forward's ``y`` bit for bit and passes that forward's own judgement (``pc.judge``);
* layer A (integers): the slot totals EQUAL the fp64 sum y and sum y**2 of the written ``y``.  Every per-channel sum of
  |y| and of y**2 is an integer below 2**24 (asserted from the reference first), so every fp32 partial sum in any
  order is exact, and so are the fp64 slot sums;
* layer B (reals): ``nm.assert_sum`` -- (chain + 4) * u * sum|term| -- with the fp64 reference and magnitudes taken from
  the ``y`` the kernel wrote and ``chain`` the launcher's own return value (checked against its formula:
  ceil(tiles / row blocks) * PT additions in a lane, 16 for the lane fold, 4 for the wave fold); then
  ``bn_finalize_slots`` on those slots against the fp64 finalize of the kernel's own totals (``nm.check_finalize``), as
  tests/test_bnact_gpu.py's ``_check_stats`` does.

The model test judges the gradients of the step with ``--native-convstats`` on against an fp64 run of the stock model:
per parameter the relative L2 error may not exceed twice that of the flag-off arm plus the fp32 u.  The two arms
differ only in the summation order of the statistics; the factor 2 is room for that reordering and nothing else.
Measured (bf16, batch 8, 32x32): see profiles/convstats_mi355x.md.
"""
import copy

import pytest
import torch
import torch.nn as nn

import _numerics as nm
import _pointwise_cases as pc
from _numerics import U

pytestmark = pytest.mark.gpu

DEV = "cuda"
EPS, MOM = 1e-5, 0.1
KERNELS = ("pwconv_fwd_stats", "pwconv_fwd", "bnact_stats")
DEFAULT_BLOCKS = 1536
_ids = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v).split(".")[-1]
ALL = pytest.mark.parametrize("g,dtype,layer", [(g, dt, la) for g in pc.GEOMS for dt in pc.DTYPES for la in pc.LAYERS],
                              ids=_ids)
CHAIN_GEOMS = [(8, 56, 56, 16, 96), (4, 28, 28, 32, 192)]  # one output slice (196 tiles), two slices (25 tiles)


def _C():
    from pytorch_distributed_template_amd.ops import native
    return native.C


def _pw():
    from pytorch_distributed_template_amd.ops import pointwise
    return pointwise


def _bn():
    from pytorch_distributed_template_amd.ops import bnact
    return bnact


def _counts():
    c = _C().dispatch_counts()
    return {k: c.get(k, 0) for k in KERNELS}


def _delta(before):
    after = _counts()
    return {k: after[k] - before[k] for k in before}


def _d(stats=0, fwd=0, bn=0):
    return {"pwconv_fwd_stats": stats, "pwconv_fwd": fwd, "bnact_stats": bn}


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def plan(M, K, max_blocks):
    """(output slices, partial rows, chain) the launcher must use: the slice width follows K alone."""
    NG, PT = (1, 4) if K <= 32 else (2, 4) if K <= 64 else (4, 2)
    nslices = -(-K // (NG * 32))
    mtiles = -(-M // (64 * PT))
    per = min(max((max_blocks or DEFAULT_BLOCKS) // nslices, 1), mtiles)
    return nslices, per, -(-mtiles // per) * PT + 16 + 4


def _run(g, dtype, layer, max_blocks=0, name=None):
    """One launch from NaN-filled buffers, every check of the module docstring; returns (y, slots)."""
    C_ = _C()
    N, H, W, C, K = g
    M = pc.rows(g)
    name = name or f"pwconv_fwd_stats {g} {dtype} {layer} max_blocks={max_blocks}"
    d = pc.case("fwd", g, dtype, layer)
    x, w = d["x"].to(DEV), d["w"].to(DEV)
    S = C_.stat_slots()
    y = _nan(N, H, W, K, dtype=dtype)
    slots = _nan(S * K * 2, dtype=torch.float64)
    before = _counts()
    rows, chain = C_.pwconv_fwd_stats(x, w, y, slots, M, C, K, max_blocks)
    assert _delta(before) == _d(stats=1)
    assert (rows, chain) == plan(M, K, max_blocks)[1:], (name, rows, chain, plan(M, K, max_blocks))
    assert torch.equal(y, _pw().pwconv_fwd(x, w)), f"{name}: y differs from pwconv_fwd's"
    pc.judge(y.cpu(), d, dtype, layer, name, "pwconv_fwd")
    assert bool(torch.isfinite(slots).all()), f"{name}: slot entries left unwritten"
    tot = slots.view(S, K, 2).sum(0)
    y64 = y.double().view(M, K)
    ref = torch.stack([y64.sum(0), (y64 * y64).sum(0)], 1)
    mag = torch.stack([y64.abs().sum(0), (y64 * y64).sum(0)], 1)
    if layer == "int":
        r64 = nm.round_exact(d["ref"], dtype).reshape(M, K)
        assert float(r64.abs().sum(0).max()) < 2 ** 24 and float((r64 * r64).sum(0).max()) < 2 ** 24, name
        nm.assert_exact(tot.cpu(), ref.cpu(), f"{name}: totals")
        return y, slots
    nm.assert_sum(tot, ref, mag, chain, f"{name}: sums", 2, family="pwconv_fwd_stats")
    gen = torch.Generator(device=DEV).manual_seed(sum(g))
    r = lambda *s: torch.rand(*s, device=DEV, generator=gen)
    gamma = (r(K) + 0.5) * torch.where(r(K) < 0.3, -1.0, 1.0)
    beta = torch.randn(K, device=DEV, generator=gen)
    rm0, rv0 = torch.randn(K, device=DEV, generator=gen), r(K) + 0.5
    rm, rv = rm0.clone(), rv0.clone()
    coef, sums = _nan(4 * K), _nan(2 * K, dtype=torch.float64)
    C_.bn_finalize_slots(slots, float(M), gamma, beta, EPS, MOM, rm, rv, coef, sums, True)
    fref = nm.bn_finalize_ref(tot[:, 0], tot[:, 1], float(M), gamma, beta, EPS, MOM, rm0, rv0)
    nm.check_finalize(coef, rm, rv, fref, K, f"{name}: finalize", family="pwconv_fwd_stats_finalize")
    return y, slots


@ALL
def test_pwconv_fwd_stats(g, dtype, layer):
    _run(g, dtype, layer)


@pytest.mark.parametrize("layer", pc.LAYERS)
@pytest.mark.parametrize("dtype", pc.DTYPES, ids=_ids)
@pytest.mark.parametrize("g", CHAIN_GEOMS, ids=_ids)
def test_chains_across_tiles(g, dtype, layer):
    """Few persistent blocks at a large M: a lane's chain runs over 25 to 196 tiles.  The returned plan follows the
    formula, the bounds hold with that chain, y does not depend on the block count, the slots repeat run to run."""
    M, K = pc.rows(g), g[4]
    nslices = plan(M, K, 0)[0]
    assert nslices == (1 if K == 96 else 2)
    ys = []
    for mb in (0, 2 * nslices, nslices):
        y, slots = _run(g, dtype, layer, mb)
        y2, slots2 = _run(g, dtype, layer, mb)
        assert torch.equal(slots, slots2) and torch.equal(y, y2)
        ys.append(y)
    assert plan(M, K, nslices)[1] == 1 and plan(M, K, nslices)[2] == (196 if K == 96 else 25) * 2 + 20
    assert torch.equal(ys[0], ys[1]) and torch.equal(ys[0], ys[2])


# (geometry, max_blocks, what it is, (M, K, partial rows) it must have)
EDGES = [
    ((1, 1, 1, 32, 16), 0, "M = 1", (1, 16, 1)),
    ((3, 9, 11, 16, 96), 0, "M = 297: a ragged last tile", (297, 96, 3)),
    ((2, 7, 9, 96, 24), 0, "N = 24 inside a 32-wide slice", (126, 24, 1)),
    ((5, 13, 13, 40, 200), 0, "N = 200: the last slice partly past N", (845, 200, 7)),
    ((1, 2, 3, 8, 2048), 3, "N = 2048, max_blocks below the 16 slices: one row block per slice", (6, 2048, 1)),
]


@pytest.mark.parametrize("layer", pc.LAYERS)
@pytest.mark.parametrize("dtype", pc.DTYPES, ids=_ids)
@pytest.mark.parametrize("g,mb,what,expect", EDGES, ids=[e[2].split(":")[0] for e in EDGES])
def test_ragged_edges(g, mb, what, expect, dtype, layer):
    M, K = pc.rows(g), g[4]
    nslices, per, _ = plan(M, K, mb)
    assert (M, K, per) == expect, what
    if mb:
        assert mb < nslices
    _run(g, dtype, layer, mb, name=f"{what} {dtype} {layer}")


def test_contract_errors():
    C_ = _C()
    S = C_.stat_slots()
    bf = dict(dtype=torch.bfloat16, device=DEV)
    x, w, y = torch.zeros(16, 16, **bf), torch.zeros(8, 16, **bf), torch.zeros(16, 8, **bf)
    ok = torch.zeros(S * 8 * 2, dtype=torch.float64, device=DEV)
    C_.pwconv_fwd_stats(x, w, y, ok, 16, 16, 8, 0)
    with pytest.raises(RuntimeError):  # slots too small
        C_.pwconv_fwd_stats(x, w, y, ok[:-1], 16, 16, 8, 0)
    with pytest.raises(RuntimeError):  # C = 12
        C_.pwconv_fwd_stats(torch.zeros(16, 12, **bf), torch.zeros(8, 12, **bf), y, ok, 16, 12, 8, 0)
    with pytest.raises(RuntimeError):  # a negative block count
        C_.pwconv_fwd_stats(x, w, y, ok, 16, 16, 8, -1)
    with pytest.raises(RuntimeError):  # mixed dtypes
        C_.pwconv_fwd_stats(x, w.half(), y, ok, 16, 16, 8, 0)


# ------------------------------------------------------------------------------------------ the pair of modules
def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _pair_models(C, K, act):
    from pytorch_distributed_template_amd.ops.convstats import convert_convstats
    torch.manual_seed(11)
    mods = [nn.Conv2d(C, K, 1, bias=False), nn.BatchNorm2d(K, eps=EPS, momentum=MOM)] + ([nn.ReLU6()] if act else [])
    base = nn.Sequential(*mods).to(DEV)
    with torch.no_grad():
        base[1].weight.copy_(torch.rand(K) + 0.5), base[1].bias.copy_(torch.randn(K))
    assert _pw().convert_pointwise(base) == 1 and _bn().convert_bnact(base) == (1, 1 if act else 0)
    fused = copy.deepcopy(base)
    assert convert_convstats(fused) == 1
    return base.train(), fused.train()


def _step(model, x_nhwc, gy_nhwc, dtype):
    model.zero_grad()
    x = _nchw(x_nhwc).detach().requires_grad_(True)
    with torch.autocast("cuda", dtype=dtype):
        out = model(x)
    res = dict(out=out.detach().clone())
    if model.training:
        out.backward(_nchw(gy_nhwc))
        res.update(dx=x.grad, dw=model[0].weight.grad.clone(), dgamma=model[1].weight.grad.clone(),
                   dbeta=model[1].bias.grad.clone())
    res.update(rm=model[1].running_mean.clone(), rv=model[1].running_var.clone(),
               nbt=model[1].num_batches_tracked.clone())
    return res


def _same(a, b, name):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), f"{name}: {k} differs"


@pytest.mark.parametrize("act", ["relu6", None])
@pytest.mark.parametrize("dtype", pc.DTYPES, ids=_ids)
def test_pair_module_path(dtype, act):
    pw, bn = _pw(), _bn()
    g = (3, 9, 11, 16, 96)
    N, H, W, C, K = g
    M = pc.rows(g)
    x_nhwc = pc.case("fwd", g, dtype, "real")["x"].to(DEV)
    gy_nhwc = pc.case("dgrad", g, dtype, "real")["dy"].to(DEV)
    base, fused = _pair_models(C, K, act)
    actname = act or "identity"

    # the functional composition on the same values
    w16 = fused[0].weight.detach().reshape(K, C).to(dtype)
    gamma, beta = fused[1].weight.detach().clone(), fused[1].bias.detach().clone()
    rm, rv = fused[1].running_mean.clone(), fused[1].running_var.clone()
    y, slots, _ = pw.pwconv_fwd_stats(x_nhwc, w16)
    coef = bn.bnact_coef_from_slots(slots, M, gamma, beta, rm, rv, EPS, MOM)
    out = bn.bnact_fwd(y, coef, actname)
    sums = bn.bnact_bwd_reduce(gy_nhwc, y, coef, actname)
    dgamma, dbeta, bcoef = bn.bnact_bwd_coef(sums, M, coef, gamma)
    dy = bn.bnact_bwd_apply(gy_nhwc, y, coef, bcoef, actname)
    want = dict(out=_nchw(out), dx=_nchw(pw.pwconv_dgrad(dy, w16)), dw=pw.pwconv_wgrad(x_nhwc, dy).view(K, C, 1, 1),
                dgamma=dgamma, dbeta=dbeta, rm=rm, rv=rv, nbt=torch.tensor(1, device=DEV))

    before = _counts()
    got = _step(fused, x_nhwc, gy_nhwc, dtype)
    assert _delta(before) == _d(stats=1)  # the conv's epilogue, neither the plain forward nor the BatchNorm's own pass
    _same(got, want, "fused pair vs the functional composition")

    # the unfused pair: bnact_stats sums in another order, so only its dispatch is pinned here
    before = _counts()
    unfused = _step(base, x_nhwc, gy_nhwc, dtype)
    assert _delta(before) == _d(fwd=1, bn=1)

    # eval mode (fresh modules: equal running statistics): the conv's plain forward, the BatchNorm on the stock ops,
    # bit for bit the unfused pair
    base2, fused2 = _pair_models(C, K, act)
    fused2.eval(), base2.eval()
    before = _counts()
    e1 = _step(fused2, x_nhwc, gy_nhwc, dtype)
    assert _delta(before) == _d(fwd=1)
    _same(e1, _step(base2, x_nhwc, gy_nhwc, dtype), "eval")
    fused2.train()

    # a forward hook added after the conversion that returns another tensor: the unfused path, bit for bit
    h = fused2[0].register_forward_hook(lambda m, i, o: o.clone())
    before = _counts()
    hooked = _step(fused2, x_nhwc, gy_nhwc, dtype)
    assert _delta(before) == _d(fwd=1, bn=1)
    _same(hooked, unfused, "hooked conv")
    h.remove()
    # a pre-hook on the BatchNorm that replaces its input: the conv has emitted, the BatchNorm does not take it
    h = fused2[1].register_forward_pre_hook(lambda m, i: (i[0].clone(),))
    before = _counts()
    hooked = _step(fused2, x_nhwc, gy_nhwc, dtype)
    assert _delta(before) == _d(stats=1, bn=1)
    h.remove()
    for k in ("out", "dx", "dw", "dgamma", "dbeta"):
        assert torch.equal(hooked[k], unfused[k]), k
    # and without hooks the pair is fused again
    before = _counts()
    _step(fused2, x_nhwc, gy_nhwc, dtype)
    assert _delta(before) == _d(stats=1)


# ------------------------------------------------------------------------------------------ MobileNetV2
def _relerr(a, ref64):
    return float((a.double().cpu() - ref64).norm() / ref64.norm().clamp_min(1e-300))


def test_mobilenet_v2_all_five_conversions():
    from pytorch_distributed_template_amd.engine.torch_trainer import TorchTrainer
    from pytorch_distributed_template_amd.models import registry
    from pytorch_distributed_template_amd.ops import depthwise, stemconv
    from pytorch_distributed_template_amd.ops.convstats import convert_convstats
    dtype = torch.bfloat16
    torch.manual_seed(0)
    base = registry.create("mobilenet_v2", dropout=0.0)
    x = torch.randn(8, 3, 32, 32)
    t = torch.randint(0, 1000, (8,))

    # fp64, stock model, same weights and batch
    m64 = copy.deepcopy(base).double().train()
    loss64 = torch.nn.functional.cross_entropy(m64(x.double()), t)
    loss64.backward()
    g64 = [p.grad for p in m64.parameters()]
    names = [n for n, _ in base.named_parameters()]

    def run(convstats):
        m = copy.deepcopy(base)
        assert depthwise.convert_depthwise(m) == 17 and _pw().convert_pointwise(m) == 34
        assert stemconv.convert_stem(m) == 1 and _bn().convert_bnact(m) == (52, 35)
        if convstats:
            assert convert_convstats(m) == 34
        tr = TorchTrainer(m, DEV, dtype=dtype)
        before = _counts()
        _, met = tr.train_step(x.to(DEV), t.to(DEV))
        torch.cuda.synchronize()
        return _delta(before), met[0].clone(), [p.grad.detach().clone() for _, p in m.named_parameters()]

    d_on, loss_on, g_on = run(True)
    assert d_on == _d(stats=34, bn=18)  # 52 BatchNorms, 34 behind a pointwise conv
    d_off, loss_off, g_off = run(False)
    assert d_off == _d(fwd=34, bn=52)
    d2, loss2, g2 = run(True)
    assert torch.equal(loss_on, loss2) and all(torch.equal(a, b) for a, b in zip(g_on, g2))  # seeded runs repeat
    assert torch.isfinite(loss_on) and all(torch.isfinite(g).all() for g in g_on)
    bad, rows = [], []
    for n, a, b, r in zip(names, g_on, g_off, g64):
        e_on, e_off = _relerr(a, r), _relerr(b, r)
        rows.append((n, e_on, e_off))
        if not e_on <= 2 * e_off + U:
            bad.append((n, e_on, e_off))
    print("relative L2 error of the gradients against fp64 (parameter, convstats on, off):")
    for n, e_on, e_off in rows:
        print(f"  {n}: {e_on:.4e} {e_off:.4e}")
    print(f"loss: on {float(loss_on):.6f} off {float(loss_off):.6f} fp64 {float(loss64.detach()):.6f}")
    print("largest relative L2 distance between the two arms' gradients:",
          max(_relerr(a, b.double().cpu()) for a, b in zip(g_on, g_off)))
    assert not bad, bad
