"""Fused BatchNorm + activation HIP kernels (csrc/kernels/bnact.hip), the ``BNAct2d`` module and a converted MobileNetV2
training step on an MI355X, in bf16 and fp16.

Every reference is fp64 and is computed from the very 16-bit / fp32 values the kernel reads; every tolerance is one of
the derived bounds of tests/_bnact_numerics.py and tests/_numerics.py (u = 2**-24):

* bnact_fwd, bnact_bwd_apply: half a 16-bit ulp at |ref| + 8u * mag per element;
* bnact_stats, bnact_bwd_reduce: (n_chain + 4) * u * sum|term| per channel and sum, n_chain = ceil(rows / (blocks *
  lanes)) + lanes from the (blocks, lanes) the launcher returns;
* the finalize outputs (bn_finalize_slots, bn_bwd_finalize): check_finalize / check_bwd_finalize against the fp64
  finalize of the kernel's own sums (each stage is judged from the previous stage's actual outputs).

Output buffers start as NaN, so an element a kernel does not write fails its bound.  Coefficients differ per channel;
channel 0 of x is constant (variance exactly 0), channel 1 of the coefficients is scaled by 1e-6 (fp16 outputs in the
subnormal range).  Seeds are chosen (a reseed loop) so that no reference u lies within 8u * mag_u of a breakpoint
(0, 6, -3, 3) of any activation, so no element is excluded from any check; the tests assert that count is 0.  Among
the 33.5 million elements of the nontemporal case some always fall into a band (about 4e-7 per element and
breakpoint): there the input is changed at those positions (x * 0.75) until none does.
"""
import copy

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import _bnact_numerics as bm
import _numerics as nm
from _numerics import U

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
ACTS = bm.ACTS
EPS, MOM = 1e-5, 0.1
KERNELS = ("bnact_stats", "bnact_fwd", "bnact_bwd_reduce", "bnact_bwd_apply")

# (N, H, W, C)
SHAPES = [
    (2, 1, 1, 8),       # 2 rows, minimum C
    (2, 7, 7, 8),
    (3, 9, 11, 24),     # C / 8 = 3 does not divide the block: 85 row lanes, one idle thread
    (2, 17, 17, 96),    # 12 channel groups x 21 row lanes
    (2, 5, 6, 144),
    (2, 2, 2, 960),     # 120 groups: 4 column chunks of 30
    (2, 7, 7, 1280),    # 160 groups: 5 column chunks of 32 x 8 row lanes
    (2, 3, 3, 2048),    # the widest: 256 groups, one row lane
    (4, 28, 28, 32),    # several row blocks and thread chains longer than 1
]
# one operand of 64 MiB + 1.6 KB: the nontemporal instantiations (per-dtype activation to bound the test time)
NT_SHAPE = (1, 1, 174767, 192)
NT_ACT = {torch.bfloat16: "hardswish", torch.float16: "relu6"}


def _C():
    from pytorch_distributed_template_amd.ops import native
    return native.C


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def _counts():
    c = _C().dispatch_counts()
    return {k: c.get(k, 0) for k in KERNELS}


def _delta(before):
    after = _counts()
    return {k: after[k] - before[k] for k in before}


def _each(n):
    return {k: n for k in KERNELS}


_cache = {}


def _in_bands(x, coef, C, fix):
    """How many reference u of x [rows, C] lie in a breakpoint band of any activation; ``fix`` (the one large case):
    change x there, up to 10 times, until none does."""
    total = 0
    for _ in range(10 if fix else 1):
        total = 0
        for sl in _row_chunks(x.shape[0], C):
            u, mag_u = bm.u_ref(x[sl], coef, C)
            near = torch.zeros_like(u, dtype=torch.bool)
            for a in ACTS:
                near |= bm.near_breakpoint(u, mag_u, a)
            n = int(near.sum())
            total += n
            if n and fix:
                x[sl] = torch.where(near, (x[sl].float() * 0.75).to(x.dtype), x[sl])
        if total == 0:
            break
    return total


def _data(shape, dtype):
    """Inputs of one case on the GPU (shared, read-only): x, g [N, H, W, C] 16-bit, coef [4C], bcoef [3C], and how many
    reference u fall into a breakpoint band (0 for the seed kept)."""
    key = (shape, dtype)
    if key in _cache:
        return _cache[key]
    N, H, W, C = shape
    rows = N * H * W
    for attempt in range(1000):
        gen = torch.Generator(device=DEV).manual_seed(4321 + 31 * (sum(shape) + C) + (dtype == torch.float16) + 1000 * attempt)
        r = lambda *s: torch.rand(*s, device=DEV, generator=gen)
        rn = lambda *s: torch.randn(*s, device=DEV, generator=gen)
        std, mean = r(C) * 3, r(C) * 10 - 5
        std[0] = 0.0  # a constant channel: variance exactly 0
        x = (rn(rows, C) * std + mean).to(dtype)
        g = rn(rows, C).to(dtype)
        sign = torch.where(r(C) < 0.3, -1.0, 1.0)
        coef = torch.cat([(r(C) + 0.5) * sign, rn(C) * 0.3, rn(C) * 0.3, r(C) + 0.5]).contiguous()
        bcoef = torch.cat([(r(C) + 0.5) * sign, rn(C) * 0.2, rn(C) * 0.1]).contiguous()
        coef[1] *= 1e-6  # channel 1 tiny: fp16 outputs in the subnormal range
        coef[C + 1] *= 1e-6
        for k in range(3):
            bcoef[k * C + 1] *= 1e-6
        excluded = _in_bands(x, coef, C, fix=rows * C > 1 << 22)
        if excluded == 0:
            break
    else:
        raise AssertionError(f"no seed keeps every u of {shape} {dtype} out of the breakpoint bands")
    d = dict(x=x.view(N, H, W, C), g=g.view(N, H, W, C), coef=coef, bcoef=bcoef, rows=rows, C=C, excluded=excluded,
             seed_attempt=attempt)
    if rows * C <= 1 << 20:
        _cache[key] = d
    return d


def _row_chunks(rows, C, elems=1 << 22):
    step = max(1, elems // C)
    for lo in range(0, rows, step):
        yield slice(lo, min(rows, lo + step))


# ------------------------------------------------------------------------------------------------ direct kernel calls
def _check_stats(x, rows, C, name, family="bnact_stats"):
    """bnact_stats -> slots against the fp64 sums (sum bound), then bn_finalize_slots against the fp64 finalize of the
    kernel's own sums (check_finalize).  Returns coef."""
    C_ = _C()
    S = C_.stat_slots()
    slots = _nan(S * C * 2, dtype=torch.float64)
    blocks, lanes = C_.bnact_stats(x, slots, rows, C)
    assert bool(torch.isfinite(slots).all()), f"{name}: slot entries left unwritten"
    tot = slots.view(S, C, 2).sum(0)
    x2 = x.view(rows, C)
    ref = torch.zeros(C, 2, dtype=torch.float64, device=DEV)
    mag = torch.zeros(C, 2, dtype=torch.float64, device=DEV)
    for sl in _row_chunks(rows, C):
        x64 = x2[sl].double()
        ref[:, 0] += x64.sum(0)
        ref[:, 1] += (x64 * x64).sum(0)
        mag[:, 0] += x64.abs().sum(0)
        mag[:, 1] += (x64 * x64).sum(0)
    chain = bm.n_chain(rows, blocks, lanes)
    nm.assert_sum(tot, ref, mag, chain, f"{name}: sums", 2, family=family)
    gamma = (torch.rand(C, device=DEV) + 0.5) * torch.where(torch.rand(C, device=DEV) < 0.3, -1.0, 1.0)
    beta = torch.randn(C, device=DEV)
    rm0, rv0 = torch.randn(C, device=DEV), torch.rand(C, device=DEV) + 0.5
    rm, rv = rm0.clone(), rv0.clone()
    coef, sums = _nan(4 * C), _nan(2 * C, dtype=torch.float64)
    C_.bn_finalize_slots(slots, float(rows), gamma, beta, EPS, MOM, rm, rv, coef, sums, True)
    fref = nm.bn_finalize_ref(tot[:, 0], tot[:, 1], float(rows), gamma, beta, EPS, MOM, rm0, rv0)
    nm.check_finalize(coef, rm, rv, fref, C, f"{name}: finalize", family=family)
    # against the exact statistics: the mean moves by the sum's error / rows on top of its rounding; the constant
    # channel's exact variance is 0
    exact_mean = ref[:, 0] / rows
    nm.assert_within(coef[2 * C:3 * C], exact_mean, 2 * U * exact_mean.abs() + (chain + 4) * U * mag[:, 0] / rows,
                     f"{name}: mean vs exact", C, family=family)
    return coef, (blocks, lanes)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_bnact_stats(shape, dtype):
    d = _data(shape, dtype)
    assert d["excluded"] == 0
    x = d["x"]
    assert bool((x.view(-1, d["C"])[:, 0] == x.view(-1, d["C"])[0, 0]).all())  # the constant channel
    torch.manual_seed(sum(shape))
    _check_stats(x, d["rows"], d["C"], f"bnact_stats {shape} {dtype}")


def _check_kernels(d, act, dtype, name, chunked=False):
    """bnact_fwd, bnact_bwd_reduce (through bn_slot_sum) and bnact_bwd_apply of one case against fp64."""
    C_ = _C()
    x, g, coef, bcoef, rows, C = d["x"], d["g"], d["coef"], d["bcoef"], d["rows"], d["C"]
    a = ACTS.index(act)
    x2, g2 = x.view(rows, C), g.view(rows, C)
    chunks = list(_row_chunks(rows, C)) if chunked else [slice(0, rows)]
    # forward
    out = torch.full_like(x, float("nan"))
    C_.bnact_fwd(x, coef, out, rows, C, a)
    for sl in chunks:
        bm.assert_fwd(out.view(rows, C)[sl], x2[sl], coef, C, act, dtype, name=f"{name}: fwd rows {sl.start}..",
                      family="bnact_fwd")
    # backward reduce
    S = C_.stat_slots()
    slots = _nan(S * C * 2, dtype=torch.float64)
    blocks, lanes = C_.bnact_bwd_reduce(g, x, coef, slots, rows, C, a)
    assert bool(torch.isfinite(slots).all()), f"{name}: slot entries left unwritten"
    sums = _nan(2 * C, dtype=torch.float64)
    C_.bn_slot_sum(slots, C, 2, sums)
    ref = torch.zeros(C, 2, dtype=torch.float64, device=DEV)
    mag = torch.zeros(C, 2, dtype=torch.float64, device=DEV)
    for sl in chunks:
        r_, m_ = bm.bwd_reduce_ref(g2[sl], x2[sl], coef, C, act)
        ref += r_
        mag += m_
    nm.assert_sum(sums.view(2, C).t(), ref, mag, bm.n_chain(rows, blocks, lanes), f"{name}: bwd sums", 2,
                  family="bnact_bwd_reduce")
    # backward apply
    dx = torch.full_like(x, float("nan"))
    C_.bnact_bwd_apply(g, x, coef, bcoef, dx, rows, C, a)
    for sl in chunks:
        bm.assert_bwd_apply(dx.view(rows, C)[sl], g2[sl], x2[sl], coef, bcoef, C, act, dtype,
                            name=f"{name}: bwd apply rows {sl.start}..", family="bnact_bwd_apply")
    return out, dx


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_kernels_against_fp64(shape, act, dtype):
    d = _data(shape, dtype)
    assert d["excluded"] == 0  # nothing near a breakpoint: no element leaves any check
    before = _counts()
    out, _ = _check_kernels(d, act, dtype, f"{shape} {act} {dtype}")
    assert _delta(before) == {"bnact_stats": 0, "bnact_fwd": 1, "bnact_bwd_reduce": 1, "bnact_bwd_apply": 1}
    if dtype == torch.float16 and d["rows"] >= 8:
        assert bool((out.view(-1, d["C"])[:, 1].float().abs() < 2.0 ** -14).any())  # subnormal outputs were exercised


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_kernels_nontemporal(dtype):
    """Operands of 64 MiB and more take the nontemporal instantiations: all four kernels at (174767, 192)."""
    d = _data(NT_SHAPE, dtype)
    assert d["rows"] * d["C"] * 2 >= 64 << 20 and d["excluded"] == 0
    torch.manual_seed(3)
    _check_stats(d["x"], d["rows"], d["C"], f"bnact_stats NT {dtype}")
    _check_kernels(d, NT_ACT[dtype], dtype, f"NT {NT_ACT[dtype]} {dtype}", chunked=True)
    del d
    torch.cuda.empty_cache()


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("act", ["relu", "relu6", "hardswish"])
def test_exact_breakpoints_equal_torch_bit_for_bit(act, dtype):
    """scale = 1, shift = 0, x in {-3, 0, 3, 6}: u = x exactly, and the forward and the backward (A = 1, B = Cc = 0:
    dx = dz) equal torch's activation and its autograd bit for bit, at every breakpoint.  Only the sign of a zero is
    left out of the comparison: torch's own kernels disagree on it (hardswish(-3) = -3 * 0 / 6 is -0.0 from its CPU
    kernels and its bf16 GPU kernel, as from bnact_fwd, but +0.0 from its fp16 GPU kernel)."""
    C_ = _C()
    C, rows = 8, 64
    fn = {"relu": F.relu, "relu6": F.relu6, "hardswish": F.hardswish}[act]
    x = torch.tensor([-3.0, 0.0, 3.0, 6.0], device=DEV).repeat(rows * C // 4).to(dtype).view(rows, C)
    torch.manual_seed(11)
    g = ((torch.rand(rows, C, device=DEV) + 0.5) * torch.where(torch.rand(rows, C, device=DEV) < 0.5, -1.0, 1.0)).to(dtype)
    one, zero = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
    coef, bcoef = torch.cat([one, zero, zero, one]), torch.cat([one, zero, zero])
    out, dx = torch.full_like(x, float("nan")), torch.full_like(x, float("nan"))
    C_.bnact_fwd(x, coef, out, rows, C, ACTS.index(act))
    C_.bnact_bwd_apply(g, x, coef, bcoef, dx, rows, C, ACTS.index(act))
    xr = x.clone().requires_grad_(True)
    y = fn(xr)
    y.backward(g)
    bits = lambda t: (t.detach() + 0.0).view(torch.int16)  # -0.0 + 0.0 = +0.0; every other value keeps its bits
    assert torch.equal(bits(out), bits(y)), (out[0], y[0])
    assert torch.equal(bits(dx), bits(xr.grad)), (dx[0], xr.grad[0], g[0])


def test_launchers_reject_what_they_do_not_cover():
    C_ = _C()
    x = torch.zeros(4, 16, dtype=torch.bfloat16, device=DEV)
    coef, bcoef = torch.zeros(64, device=DEV), torch.zeros(48, device=DEV)
    slots = torch.zeros(C_.stat_slots() * 16 * 2, dtype=torch.float64, device=DEV)
    out = torch.full_like(x, float("nan"))
    before = _counts()
    with pytest.raises(RuntimeError, match="act must be"):
        C_.bnact_fwd(x, coef, out, 4, 16, 4)
    with pytest.raises(RuntimeError, match="multiple of 8"):
        C_.bnact_fwd(torch.zeros(2, 12, dtype=torch.bfloat16, device=DEV), coef, out, 2, 12, 0)
    with pytest.raises(RuntimeError, match="multiple of 8"):
        C_.bnact_stats(torch.zeros(2, 2056, dtype=torch.bfloat16, device=DEV), slots, 2, 2056)
    with pytest.raises(RuntimeError, match="mixed dtypes"):
        C_.bnact_bwd_reduce(x.half(), x, coef, slots, 4, 16, 1)
    with pytest.raises(RuntimeError, match="must hold"):
        C_.bnact_bwd_apply(x, x, coef, bcoef, out, 8, 16, 1)
    with pytest.raises(RuntimeError, match="float32"):
        C_.bnact_fwd(x, coef.double(), out, 4, 16, 0)
    torch.cuda.synchronize()
    assert _delta(before) == _each(0) and bool(torch.isnan(out.float()).all())  # nothing ran


# ------------------------------------------------------------------------------------------------------- the module
def _stock(C, act):
    return nn.Sequential(nn.BatchNorm2d(C), {"identity": nn.Identity(), "relu": nn.ReLU(), "relu6": nn.ReLU6(),
                                             "hardswish": nn.Hardswish()}[act])


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("act", ACTS)
def test_module_chain_against_fp64(act, dtype):
    """``BNAct2d`` under autocast on (3, 24, 9, 11), two steps.  The module's outputs are bitwise those of the functional
    ops (the kernels are deterministic), so every stage is judged against fp64 from the previous stage's actual
    outputs: statistics -> coefficients and running statistics (unbiased variance) -> output -> backward sums ->
    dgamma / dbeta / bcoef -> dx.  The stage formulas themselves, evaluated in fp64 with exact statistics, equal
    ``BatchNorm2d`` + activation under torch.autograd in fp64 on the same rounded inputs to 1e-9, and the module's
    output stays within its bound of that autograd forward once the measured coefficient differences are propagated
    (|x| |dscale| + |dshift|, times the activation's Lipschitz constant 1.5)."""
    from pytorch_distributed_template_amd.ops import bnact
    from pytorch_distributed_template_amd.optim.flat import FlatParams
    shape = (3, 9, 11, 24)
    d = _data(shape, dtype)
    N, H, W, C = shape
    rows = d["rows"]
    torch.manual_seed(5 + ACTS.index(act))
    model = nn.Sequential(bnact.BNAct2d(C, eps=EPS, momentum=MOM, act=act))
    m = model[0]
    with torch.no_grad():
        m.weight.copy_((torch.rand(C) + 0.5) * torch.where(torch.rand(C) < 0.3, -1.0, 1.0))
        m.bias.copy_(torch.randn(C) * 0.5)
        m.running_mean.copy_(torch.randn(C))
        m.running_var.copy_(torch.rand(C) + 0.5)
    model.to(DEV)
    rm_init, rv_init = m.running_mean.clone(), m.running_var.clone()
    flat = FlatParams(model, torch.device(DEV), None)
    view_w, view_b = m.weight.grad, m.bias.grad
    gamma, beta = m.weight.detach(), m.bias.detach()
    xh = d["x"]
    gh = d["g"]
    x64 = xh.double().view(rows, C)
    eps32 = float(torch.tensor(EPS).float())
    for step in (1, 2):
        rm0, rv0 = m.running_mean.clone(), m.running_var.clone()
        x = xh.permute(0, 3, 1, 2).detach().requires_grad_(True)  # NHWC storage seen as NCHW: dense channels_last
        assert x.is_contiguous(memory_format=torch.channels_last)
        before = _counts()
        with torch.autocast("cuda", dtype=dtype):
            y = m(x)
        assert _delta(before) == {"bnact_stats": 1, "bnact_fwd": 1, "bnact_bwd_reduce": 0, "bnact_bwd_apply": 0}
        assert y.dtype == dtype and y.shape == x.shape and y.is_contiguous(memory_format=torch.channels_last)
        assert int(m.num_batches_tracked) == step
        y.backward(gh.permute(0, 3, 1, 2).contiguous())  # NCHW-contiguous: backward makes it channels_last itself
        assert _delta(before) == _each(1)
        # stage 1: statistics -> coefficients, running statistics
        S = _C().stat_slots()
        slots = _nan(S * C * 2, dtype=torch.float64)
        blocks, lanes = _C().bnact_stats(xh, slots, rows, C)
        chain = bm.n_chain(rows, blocks, lanes)
        tot = slots.view(S, C, 2).sum(0)
        nm.assert_sum(tot, torch.stack([x64.sum(0), (x64 * x64).sum(0)], 1),
                      torch.stack([x64.abs().sum(0), (x64 * x64).sum(0)], 1), chain, "module: sums", 2, family="module")
        rm1, rv1 = rm0.clone(), rv0.clone()
        coef = bnact.bnact_stats(xh, gamma, beta, rm1, rv1, EPS, MOM)
        assert torch.equal(rm1, m.running_mean) and torch.equal(rv1, m.running_var)
        fref = nm.bn_finalize_ref(tot[:, 0], tot[:, 1], float(rows), gamma, beta, EPS, MOM, rm0, rv0)
        nm.check_finalize(coef, m.running_mean, m.running_var, fref, C, "module: finalize", family="module")
        # stage 2: output
        yh = y.detach().permute(0, 2, 3, 1)
        assert torch.equal(yh, bnact.bnact_fwd(xh, coef, act))
        bm.assert_fwd(yh, xh, coef, C, act, dtype, name="module: out", family="module")
        # stage 3: backward sums -> dgamma, dbeta, bcoef
        sums = bnact.bnact_bwd_reduce(gh, xh, coef, act)
        bm.assert_bwd_sums(sums.view(2, C).t(), gh, xh, coef, C, act, chain, name="module: bwd sums", family="module")
        dgamma, dbeta, bcoef = bnact.bnact_bwd_coef(sums, rows, coef, gamma)
        bref = nm.bn_bwd_finalize_ref(sums[:C], sums[C:], float(rows), coef, gamma, 1.0, C)
        nm.check_bwd_finalize(bcoef, dgamma, dbeta, bref, C, "module: bwd finalize", family="module")
        # gradients land in (and accumulate into) the flat views: the same batch twice doubles them exactly
        assert m.weight.grad is view_w and m.bias.grad is view_b
        assert dgamma.dtype == torch.float32
        assert torch.equal(flat.grad_flat(m.weight), dgamma * step) and torch.equal(flat.grad_flat(m.bias), dbeta * step)
        # stage 4: dx
        dxh = x.grad.permute(0, 2, 3, 1)
        assert x.grad.dtype == dtype and torch.equal(dxh, bnact.bnact_bwd_apply(gh, xh, coef, bcoef, act))
        bm.assert_bwd_apply(dxh, gh, xh, coef, bcoef, C, act, dtype, name="module: dx", family="module")
    # torch.autograd in fp64 on the same rounded inputs: BatchNorm2d + activation, on the CPU (torch's fp64 GPU
    # hardswish multiplies by a single-precision 1/6 and is only accurate to 1e-7)
    stock = _stock(C, act).double()
    with torch.no_grad():
        stock[0].weight.copy_(gamma.double())
        stock[0].bias.copy_(beta.double())
        stock[0].running_mean.copy_(rm_init.double())
        stock[0].running_var.copy_(rv_init.double())
    stock[0].eps, stock[0].momentum = eps32, float(torch.tensor(MOM).float())
    xa = xh.double().cpu().permute(0, 3, 1, 2).requires_grad_(True)
    ya = stock(xa)
    ya.backward(gh.double().cpu().permute(0, 3, 1, 2))
    on_gpu = lambda t: t.detach().to(DEV)
    # the stage formulas in fp64 with exact statistics are that autograd
    mean = x64.mean(0)
    var = x64.var(0, unbiased=False)
    invstd = 1.0 / torch.sqrt(var + eps32)
    scale = gamma.double() * invstd
    coef64 = torch.cat([scale, beta.double() - mean * scale, mean, invstd])
    u64 = x64 * coef64[:C] + coef64[C:2 * C]
    assert (bm.act_ref(u64, act) - on_gpu(ya).permute(0, 2, 3, 1).reshape(rows, C)).abs().max().item() < 1e-9
    dz64 = gh.double().view(rows, C) * bm.dact_ref(u64, act)
    xhat = (x64 - mean) * invstd
    r64 = nm.bn_bwd_finalize_ref(dz64.sum(0), (dz64 * xhat).sum(0), float(rows), coef64, gamma.double(), 1.0, C)
    dx64 = r64["A"] * dz64 + r64["B"] * x64 + r64["Cc"]
    assert (dx64 - on_gpu(xa.grad).permute(0, 2, 3, 1).reshape(rows, C)).abs().max().item() < 1e-9
    assert (r64["dgamma"] - on_gpu(stock[0].weight.grad)).abs().max().item() < 1e-9
    assert (r64["dbeta"] - on_gpu(stock[0].bias.grad)).abs().max().item() < 1e-9
    # the running statistics after the second step are F.batch_norm's (unbiased variance) after two updates.  Per
    # update: the 6u(|old| + |new|) of check_finalize, plus momentum times the statistic's own error -- the mean
    # moves by at most (chain + 4)u E|x|, the variance sum x^2 / n - mean^2 by at most 3 (chain + 4)u E[x^2]
    # (|mean| E|x| <= E[x^2]), times n / (n - 1)
    stock(xa.detach())
    ex, ex2 = x64.abs().mean(0), (x64 * x64).mean(0)
    nm.assert_within(m.running_mean, on_gpu(stock[0].running_mean),
                     2 * (6 * U * (rm_init.double().abs() + mean.abs()) + (chain + 4) * U * MOM * ex),
                     "module: running_mean vs F.batch_norm", C, family="module")
    nm.assert_within(m.running_var, on_gpu(stock[0].running_var),
                     2 * (6 * U * (rv_init.double().abs() + var * rows / (rows - 1))
                          + 3 * (chain + 4) * U * MOM * ex2 * rows / (rows - 1)),
                     "module: running_var vs F.batch_norm", C, family="module")
    assert int(stock[0].num_batches_tracked) == int(m.num_batches_tracked) == 2
    # the module's output against the autograd forward, the measured coefficient differences propagated
    _, mag_u, _, mag = bm.fwd_ref(xh, coef, C, act)
    ref_out = bm.act_ref(u64, act)
    slack = 1.5 * (x64.abs() * (coef[:C].double() - coef64[:C]).abs() + (coef[C:2 * C].double() - coef64[C:2 * C]).abs())
    # (the half ulp is taken at |ref| + slack: the value the kernel rounds is that far from the autograd value)
    nm.assert_within(yh.reshape(rows, C), ref_out, nm.half_ulp16(ref_out.abs() + slack, dtype) + 8 * U * mag + slack,
                     "module: out vs autograd", C, family="module")


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_module_without_input_gradient_skips_the_apply_pass(dtype):
    from pytorch_distributed_template_amd.ops import bnact
    d = _data((2, 17, 17, 96), dtype)
    m = bnact.BNAct2d(96, act="relu6").to(DEV)
    before = _counts()
    with torch.autocast("cuda", dtype=dtype):
        y = m(d["x"].permute(0, 3, 1, 2))
    y.backward(d["g"].permute(0, 3, 1, 2))
    assert _delta(before) == {"bnact_stats": 1, "bnact_fwd": 1, "bnact_bwd_reduce": 1, "bnact_bwd_apply": 0}
    assert m.weight.grad.dtype == torch.float32 and bool(torch.isfinite(m.weight.grad).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("act", ACTS)
def test_module_fallbacks(act, dtype):
    """fp32 input, NCHW 16-bit input, eval mode, C = 58 and a 1-row batch launch none of the four kernels and equal the
    stock modules (or raise the same error).

    For C = 58 the stock operator is not executed here: on the MI355X test machine torch's own training-mode
    ``torch.batch_norm`` ended the process with a segmentation fault on a 16-bit channels_last input with 58 channels
    (inside the library, before this module's code is involved again).  The test asserts instead that the module
    hands exactly that input to ``nn.BatchNorm2d.forward`` and applies the activation to what comes back; that a
    58-channel ``BNAct2d`` equals the stock modules is asserted on the CPU (tests/test_bnact_cpu.py)."""
    from unittest import mock
    from pytorch_distributed_template_amd.ops import bnact
    torch.manual_seed(5)

    def pair(C):
        a = bnact.BNAct2d(C, act=act).to(DEV)
        b = _stock(C, act).to(DEV)
        with torch.no_grad():
            a.weight.copy_(torch.rand(C) + 0.5)
            a.bias.copy_(torch.randn(C))
        b[0].load_state_dict(a.state_dict())
        return a, b

    def same(a, b, x, autocast=True):
        with torch.autocast("cuda", dtype=dtype, enabled=autocast):
            ya, yb = a(x), b(x)
        assert ya.dtype == yb.dtype and torch.equal(ya, yb)
        for k, v in a.state_dict().items():
            assert torch.equal(v, b[0].state_dict()[k]), k

    before = _counts()
    cl = lambda t: t.contiguous(memory_format=torch.channels_last)
    a, b = pair(32)
    same(a, b, cl(torch.randn(2, 32, 9, 9, device=DEV)), autocast=False)  # fp32 (the torch engine's validation)
    x16 = torch.randn(2, 32, 9, 9, device=DEV).to(dtype)  # NCHW-contiguous
    assert not x16.is_contiguous(memory_format=torch.channels_last)
    same(a, b, x16)
    a.eval(), b.eval()
    same(a, b, cl(x16))  # eval mode
    a58 = bnact.BNAct2d(58, act=act).to(DEV)  # 58 channels: no multiple of 8
    x58 = cl(torch.randn(2, 58, 9, 9, device=DEV).to(dtype))
    assert not bnact.qualifies(a58)
    seen = []
    with mock.patch.object(nn.BatchNorm2d, "forward", lambda self, inp: (seen.append((self, inp)), inp * 2)[1]):
        with torch.autocast("cuda", dtype=dtype):
            y58 = a58(x58)
    assert len(seen) == 1 and seen[0][0] is a58 and seen[0][1] is x58
    assert torch.equal(y58, _stock(58, act)[1](x58 * 2))
    a, b = pair(32)
    one = cl(torch.randn(1, 32, 1, 1, device=DEV).to(dtype))  # one value per channel: the stock error
    with torch.autocast("cuda", dtype=dtype):
        with pytest.raises(ValueError) as ea:
            a(one)
        with pytest.raises(ValueError) as eb:
            b(one)
    assert str(ea.value) == str(eb.value) and "more than 1 value per channel" in str(ea.value)
    assert _delta(before) == _each(0)
    # and the same module does take the kernels on a qualifying input
    with torch.autocast("cuda", dtype=dtype):
        a(cl(x16))
    assert _delta(before) == {"bnact_stats": 1, "bnact_fwd": 1, "bnact_bwd_reduce": 0, "bnact_bwd_apply": 0}


# ------------------------------------------------------------------------------------------------- the training step
def _relnorm(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-12)).item()


_steps = {}


def _step_refs(dtype):
    """The fp32 and the stock autocast step of MobileNetV2 (dropout 0) at 8 x 3 x 64 x 64, computed once per dtype."""
    if dtype in _steps:
        return _steps[dtype]
    from pytorch_distributed_template_amd.engine.torch_trainer import TorchTrainer
    from pytorch_distributed_template_amd.models import registry
    torch.manual_seed(0)
    base = registry.create("mobilenet_v2", dropout=0.0)
    x = torch.randn(8, 3, 64, 64, device=DEV)
    t = torch.randint(0, 1000, (8,), device=DEV)

    def run(model, dt):
        tr = TorchTrainer(model, DEV, dtype=dt)
        logits, met = tr.train_step(x, t)
        torch.cuda.synchronize()
        return tr, logits, [p.grad.detach().clone() for _, p in model.named_parameters()]

    _, l32, g32 = run(copy.deepcopy(base), torch.float32)
    _, l16, g16 = run(copy.deepcopy(base), dtype)
    _steps[dtype] = dict(base=base, x=x, t=t, run=run, l32=l32, g32=g32, l16=l16, g16=g16)
    return _steps[dtype]


@pytest.mark.parametrize("with_depthwise", [False, True], ids=["bnact", "bnact+depthwise"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_mobilenet_v2_train_step(dtype, with_depthwise):
    """One torch-engine train step of MobileNetV2 (dropout 0) with ``convert_bnact`` applied, alone and together with
    ``convert_depthwise``, against the same step in fp32 and judged against the stock autocast step exactly as
    tests/test_depthwise_gpu.py::test_mobilenet_v2_train_step does (margins 1.5x + 0.02 for the logits, 1.5x + 0.01 for
    every gradient; the 17 analytically-zero projection-BN biases measured against the gradient norm of the same
    BatchNorm's scale).

    Observed on an MI355X: the four cases passed in two of three whole-file runs; in the third, fp16 with both
    conversions missed the gradient margin on one parameter, the stem BatchNorm's scale ('features.0.1.weight': 1.479
    native against 0.853 stock autocast, margin 1.29) -- a gradient the stock fp16 step itself gets 85 % wrong.  Per
    layer the fused kernels are closer to fp64 than the stock ops (profiles/bnact_mi355x.md)."""
    from pytorch_distributed_template_amd.ops import bnact
    from pytorch_distributed_template_amd.ops import depthwise as dw
    r = _step_refs(dtype)
    base, x, t, l32, g32, l16, g16 = r["base"], r["x"], r["t"], r["l32"], r["g32"], r["l16"], r["g16"]
    mnat = copy.deepcopy(base)
    assert bnact.convert_bnact(mnat) == (52, 35)
    if with_depthwise:
        assert dw.convert_depthwise(mnat) == 17
    names = [n for n, _ in base.named_parameters()]
    assert [n for n, _ in mnat.named_parameters()] == names
    before = _counts()
    dcount = _C().dispatch_counts().get("dwconv_fwd", 0)
    tr, lnat, gnat = r["run"](mnat, dtype)
    assert _delta(before) == _each(52)  # one of each kernel per module: no silent fallback
    assert _C().dispatch_counts().get("dwconv_fwd", 0) - dcount == (17 if with_depthwise else 0)
    ours, theirs = _relnorm(lnat, l32), _relnorm(l16, l32)
    print(f"logits: native {ours:.4e}, autocast {theirs:.4e}")
    assert torch.isfinite(lnat).all()
    assert ours < 1.5 * theirs + 0.02
    # the shift of every linear bottleneck's projection BatchNorm has an analytically zero gradient (it feeds a
    # convolution followed by a training-mode BatchNorm): the error IS the gradient, measured against the gradient
    # norm of the same BatchNorm's scale (tests/test_depthwise_gpu.py)
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
    nbn = 0
    for m in mnat.modules():
        if isinstance(m, bnact.BNAct2d):
            gw = tr.flat.grad_flat(m.weight)
            assert gw.dtype == torch.float32 and torch.isfinite(gw).all() and (gw != 0).any()
            assert int(m.num_batches_tracked) == 1
            nbn += 1
    assert nbn == 52
    # validation runs in fp32 without autocast, in eval mode: every module falls back
    before = _counts()
    out, met = tr.eval_step(x, t)
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and torch.isfinite(met).all()
    assert _delta(before) == _each(0)
