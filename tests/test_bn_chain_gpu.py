"""The BatchNorm kernel chain per element against fp64, in bf16, fp16 and fp32, at every dispatched variant.

Forward: slots -> bn_finalize / bn_finalize_slots (-> bn_eval_coef, bias_coef) -> bn_apply; backward: bn_bwd_reduce ->
bn_slot_sum -> bn_bwd_finalize / bn_bwd_finalize_slots -> bn_bwd_apply; and the fp32 family.  Every reference is fp64
computed from the very 16-bit / fp32 values the kernel reads; every tolerance is one of the derived bounds of
tests/_numerics.py (u = 2**-24):

* elementwise outputs (bn_apply, bn_bwd_apply, *32): half a 16-bit ulp at |ref| + 8u * (sum of |terms|);
* reduce sums: (n_chain + 4) * u * sum|term| with n_chain = ceil(rows / (blocks * rpi)) + rpi -- a thread's chain over
  its rows, then the fp32 sum over the block's rpi row lanes; block partials are summed in fp64;
* finalize outputs: 2u .. 8u of the magnitudes of their terms (check_finalize / check_bwd_finalize).

Output buffers start as NaN (masks as 0xFF), so an element a kernel does not write fails its bound.  Coefficients
differ per channel, so a kernel indexing the wrong channel fails too; one channel is scaled by 1e-6 to put fp16
outputs into the subnormal range.

Worst observed error / bound on an MI355X with these seeds (information, not a threshold): 1a forward statistics to
coefficients 0.50; 1b bn_apply 0.9999 (the half-ulp term is tight by construction: a correct rounding reaches it); 1c
bn_bwd_reduce 0.013; 1d bn_bwd_finalize 0.50; 1e bn_bwd_apply 0.99999; 1f the chain in executor order 0.997 (its
elementwise stages; dgamma / dbeta against autograd far below); 1g the fp32 family 0.32.

1h, the fp32 stem tail (bn_relu_maxpool32, stem_pool_bwd_apply32, stem_pool_bwd_reduce32, stem_pack32): each against its
own fp64 reference (window maximum, scatter of the pooled gradient along the argmax bytes + ReLU mask + A*dz + B*y + C,
the sums of that dz, the bit pattern of the packed image), never against another kernel of this project.
"""
import math

import pytest
import torch
import torch.nn.functional as F

import _numerics as nm
from _numerics import U

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
EPS, MOM = 1e-5, 0.1

def _C():
    from pytorch_distributed_template_amd.ops import native
    return native.C


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def _rand16(rows, C, dtype, scale=1.0):
    return (torch.randn(rows, C, device=DEV) * scale).to(dtype)


def _signs(C):
    return torch.where(torch.rand(C, device=DEV) < 0.3, -1.0, 1.0)


def _coef4(C, tiny=True):
    """[scale | shift | mean | invstd], all different per channel; channel 1 at 1e-6 scale (fp16 subnormal outputs)."""
    c = torch.cat([(torch.rand(C, device=DEV) + 0.5) * _signs(C), torch.randn(C, device=DEV) * 0.3,
                   torch.randn(C, device=DEV) * 0.3, torch.rand(C, device=DEV) + 0.5]).contiguous()
    if tiny:
        c[1] *= 1e-6
        c[C + 1] *= 1e-6
    return c


def _bcoef(C):
    """[A | B | Cc] of the backward apply, different per channel; channel 1 tiny."""
    b = torch.cat([(torch.rand(C, device=DEV) + 0.5) * _signs(C), torch.randn(C, device=DEV) * 0.2,
                   torch.randn(C, device=DEV) * 0.1]).contiguous()
    b[1] *= 1e-6
    b[C + 1] *= 1e-6
    b[2 * C + 1] *= 1e-6
    return b


def _row_chunks(rows, C, elems=1 << 22):
    step = max(1, elems // C)
    for lo in range(0, rows, step):
        yield slice(lo, min(rows, lo + step))


_AR8 = None


def _mask_bits(mask, C):
    """uint8 bitmask [rows * C / 8] -> bool [rows, C]"""
    global _AR8
    if _AR8 is None:
        _AR8 = torch.arange(8, device=DEV, dtype=torch.uint8)
    return ((mask.reshape(-1, 1) >> _AR8) & 1).bool().reshape(-1, C)


def _slots_from_rows(x64, K=None):
    """fp64 slots [S][C][2] of a [rows, C] tensor: the rows split into S contiguous groups (sum x, sum x^2)."""
    S = _C().stat_slots()
    rows, C = x64.shape
    slots = torch.zeros(S, C, 2, dtype=torch.float64, device=DEV)
    for s in range(S):
        lo, hi = s * rows // S, (s + 1) * rows // S
        if hi > lo:
            slots[s, :, 0] = x64[lo:hi].sum(0)
            slots[s, :, 1] = (x64[lo:hi] * x64[lo:hi]).sum(0)
    return slots


# ------------------------------------------------------------------------------------------------ 1a
def _stat_input(rows, C, dtype):
    std = torch.rand(C, device=DEV) * 3
    std[0] = 0.0  # a constant channel: variance exactly 0
    mean = torch.rand(C, device=DEV) * 10 - 5
    return (torch.randn(rows, C, device=DEV) * std + mean).to(dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows", [3001, 1])
@pytest.mark.parametrize("C", [8, 200, 2048])
def test_forward_statistics_to_coefficients(C, rows, dtype):
    """bn_finalize_slots (one launch) and bn_slot_sum + bn_finalize (two) against fp64 x.mean / x.var and
    F.batch_norm's running statistics: C = 8 is a partial 64-channel block, 200 three full blocks and a partial one,
    2048 the widest; rows = 1 is count = 1 (variance 0, the biased variance kept for the running statistic).
    Bounds: check_finalize.  sums against the fp64 sum of the slots within 64 * 2**-53 * sum|slot| (a 64-term fp64
    summation), the two paths' sums within 2**-50 relative of each other."""
    torch.manual_seed(100 + C + rows)
    C_ = _C()
    x = _stat_input(rows, C, dtype)
    x64 = x.double()
    slots = _slots_from_rows(x64)
    gamma, beta = (torch.rand(C, device=DEV) + 0.5) * _signs(C), torch.randn(C, device=DEV)
    rm0, rv0 = torch.randn(C, device=DEV), torch.rand(C, device=DEV) + 0.5
    var = x64.var(0, unbiased=False) if rows > 1 else torch.zeros(C, dtype=torch.float64, device=DEV)
    ref = nm.bn_finalize_ref(x64.sum(0), (x64 * x64).sum(0), float(rows), gamma, beta, EPS, MOM, rm0, rv0, var=var)
    assert torch.allclose(ref["mean"], x64.mean(0), rtol=1e-13, atol=1e-13)
    if rows > 1:  # the reference's running statistics are F.batch_norm's (fp64)
        frm, frv = rm0.double(), rv0.double()
        F.batch_norm(x64, frm, frv, gamma.double(), beta.double(), True, float(torch.tensor(MOM).float()),
                     float(torch.tensor(EPS).float()))
        assert torch.allclose(frm, ref["rm_old"] + ref["rm_new"], rtol=1e-12, atol=1e-12)
        assert torch.allclose(frv, ref["rv_old"] + ref["rv_new"], rtol=1e-12, atol=1e-12)
    ssum, sabs = slots.sum(0), slots.abs().sum(0)
    results = []
    for path in ("fused", "two_launch"):
        for update in (True, False):
            rm, rv = rm0.clone(), rv0.clone()
            coef, sums = _nan(4 * C), _nan(2 * C, dtype=torch.float64)
            if path == "fused":
                C_.bn_finalize_slots(slots, float(rows), gamma, beta, EPS, MOM, rm, rv, coef, sums, update)
            else:
                C_.bn_slot_sum(slots, C, 2, sums)
                C_.bn_finalize(sums, float(rows), gamma, beta, EPS, MOM, rm, rv, coef, update)
            name = f"{path} C={C} rows={rows} update={update}"
            nm.check_finalize(coef, rm if update else None, rv if update else None, ref, C, name, family="1a")
            if not update:
                assert torch.equal(rm, rm0) and torch.equal(rv, rv0), f"{name}: running statistics were touched"
            nm.assert_within(sums.view(2, C).t(), ssum, 64 * 2.0 ** -53 * sabs, f"{name}: sums", 2, family="1a")
            results.append(sums)
    assert bool(((results[0] - results[2]).abs() <= 2.0 ** -50 * results[0].abs()).all()), \
        "fused and two-launch sums differ by more than 2**-50 relative"
    if rows == 1:
        inv = float(1.0 / math.sqrt(float(torch.tensor(EPS).float())))
        assert torch.equal(coef[3 * C:], torch.full((C,), inv, device=DEV))


@pytest.mark.parametrize("path", ["fused", "two_launch"])
def test_finalize_clamps_a_slightly_negative_variance(path):
    """sum x^2 / count - mean^2 < 0 by cancellation (built in the slots directly): invstd = 1/sqrt(eps), no NaN."""
    C_ = _C()
    C, count = 8, 1000.0
    S = C_.stat_slots()
    slots = torch.zeros(S, C, 2, dtype=torch.float64, device=DEV)
    m = torch.arange(1, C + 1, dtype=torch.float64, device=DEV) * 0.75
    slots[0, :, 0] = m * count
    slots[0, :, 1] = m * m * count * (1 - 2.0 ** -40 * torch.arange(1, C + 1, dtype=torch.float64, device=DEV))
    assert bool(((slots[0, :, 1] / count - (slots[0, :, 0] / count) ** 2) < 0).all())
    gamma, beta = torch.rand(C, device=DEV) + 0.5, torch.randn(C, device=DEV)
    rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    coef, sums = _nan(4 * C), _nan(2 * C, dtype=torch.float64)
    if path == "fused":
        C_.bn_finalize_slots(slots, count, gamma, beta, EPS, MOM, rm, rv, coef, sums, True)
    else:
        C_.bn_slot_sum(slots, C, 2, sums)
        C_.bn_finalize(sums, count, gamma, beta, EPS, MOM, rm, rv, coef, True)
    assert bool(torch.isfinite(coef).all() and torch.isfinite(rm).all() and torch.isfinite(rv).all())
    inv = float(1.0 / math.sqrt(float(torch.tensor(EPS).float())))
    assert torch.equal(coef[3 * C:], torch.full((C,), inv, device=DEV))
    ref = nm.bn_finalize_ref(slots[0, :, 0], slots[0, :, 1], count, gamma, beta, EPS, MOM, torch.zeros(C, device=DEV),
                             torch.ones(C, device=DEV))
    nm.check_finalize(coef, rm, rv, ref, C, f"negative variance ({path})", family="1a")


@pytest.mark.parametrize("C", [8, 200, 2048])
def test_bn_eval_coef_and_bias_coef(C):
    """bn_eval_coef: invstd = rsqrtf(var + eps) is not correctly rounded (one fp32 sum, then a few-ulp rsqrt): 8u|ref|
    for invstd and scale; shift = beta - mean * scale inherits the scale's 8u, the product and the subtraction:
    10u(|beta| + |mean * scale|); row 2 is running_mean itself.  bias_coef is exactly [1 | bias | 0 | 1]."""
    torch.manual_seed(C)
    C_ = _C()
    gamma, beta = (torch.rand(C, device=DEV) + 0.5) * _signs(C), torch.randn(C, device=DEV)
    rm, rv = torch.randn(C, device=DEV) * 2, torch.rand(C, device=DEV) * 4
    rv[0] = 0.0
    coef = _nan(4 * C)
    C_.bn_eval_coef(gamma, beta, rm, rv, EPS, coef)
    invstd = 1.0 / torch.sqrt(rv.double() + float(torch.tensor(EPS).float()))
    scale = gamma.double() * invstd
    nm.assert_within(coef[3 * C:], invstd, 8 * U * invstd.abs(), "eval invstd", C, family="1a")
    nm.assert_within(coef[:C], scale, 8 * U * scale.abs(), "eval scale", C, family="1a")
    nm.assert_within(coef[C:2 * C], beta.double() - rm.double() * scale,
                     10 * U * (beta.double().abs() + (rm.double() * scale).abs()), "eval shift", C, family="1a")
    assert torch.equal(coef[2 * C:3 * C], rm)
    bias = torch.randn(C + 3, device=DEV)
    bc = _nan(4 * C)
    C_.bias_coef(bias, bc, C)
    one, zero = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
    assert torch.equal(bc, torch.cat([one, bias[:C], zero, one]))


# ------------------------------------------------------------------------------------------------ 1b
APPLY_VARIANTS = [(0, True, False), (1, True, False), (2, True, False), (0, False, False), (1, False, False),
                  (2, False, False), (1, True, True), (2, True, True)]
# (1, 8) one vector; the others span more than 2 blocks and end in a partial block; 192 is no power of two (per-vector
# coefficients, one vector per thread), the others hoist the coefficients (4 vectors per thread)
APPLY_SHAPES = [(1, 8), (3001, 8), (517, 64), (173, 192), (13, 2048)]
NT_ROWS_C = {torch.bfloat16: (16411, 2048), torch.float16: (174767, 192)}  # >= 64 MiB: the nontemporal kernels
NT_ELEMS = 16411 * 2048  # the larger of the two, also the (16411, 2048) reduce case of both dtypes


def _check_apply(y, res, coef, rcoef, out, mask, C, resmode, relu, dtype, name):
    from pytorch_distributed_template_amd.ops import conv
    rows = y.numel() // C
    y2, o2 = y.view(rows, C), out.view(rows, C)
    r2 = res.view(rows, C) if res is not None else None
    m2 = mask.view(rows, C // 8) if mask is not None else None
    for sl in _row_chunks(rows, C):
        val, ref, mag = nm.bn_apply_ref(y2[sl], coef, r2[sl] if r2 is not None else None, rcoef, C, resmode, relu)
        nm.assert_rounded(o2[sl], ref, mag, dtype, name=f"{name} rows {sl.start}..", C=C, family="1b")
        if m2 is not None:
            assert torch.equal(m2[sl].reshape(-1), conv.pack_relu_mask(o2[sl])), f"{name}: mask != pack_relu_mask(out)"
            sure = val.abs() > nm.half_ulp16(val, dtype) + 8 * U * mag
            assert torch.equal(_mask_bits(m2[sl], C)[sure], (val > 0)[sure]), f"{name}: mask bit != (value > 0)"


def _run_apply(y, res, coef, rcoef, C, resmode, relu, wm, dtype, name):
    out = torch.full_like(y, float("nan"))
    mask = torch.full((y.numel() // 8,), 0xFF, dtype=torch.uint8, device=DEV) if wm else None
    _C().bn_apply(y, coef, res if resmode else None, rcoef if resmode == 2 else None, out, C, resmode, relu, mask)
    _check_apply(y, res if resmode else None, coef, rcoef, out, mask, C, resmode, relu, dtype, name)
    return out, mask


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", APPLY_SHAPES)
@pytest.mark.parametrize("variant", APPLY_VARIANTS)
def test_bn_apply(variant, shape, dtype):
    """out = act(y*scale + shift [+ res | + res*rscale + rshift]) rounded to 16 bits: assert_rounded with
    mag = |y*scale| + |shift| (+ |res| or |res*rscale| + |rshift|); the mask equals pack_relu_mask(out) and, where the
    pre-activation value is further from 0 than its own bound, the sign of the fp64 value."""
    resmode, relu, wm = variant
    rows, C = shape
    torch.manual_seed(rows * 7 + C + resmode)
    y, res = _rand16(rows, C, dtype, 2.0), _rand16(rows, C, dtype)
    coef, rcoef = _coef4(C), _coef4(C)[:2 * C].contiguous()
    if resmode == 1:
        res[:, 1] = (res[:, 1].float() * 1e-6).to(dtype)
    _run_apply(y, res, coef, rcoef, C, resmode, relu, wm, dtype, f"bn_apply{variant} {shape} {dtype}")


@pytest.fixture(scope="module", params=DTYPES, ids=["bf16", "fp16"])
def nt(request):
    """One set of >= 64 MiB tensors per dtype, shared by the nontemporal apply / backward-apply cases and the
    (16411, 2048) reduce case: y, res (also the second branch's y), g, a random mask, coefficients."""
    dtype = request.param
    torch.manual_seed(77)
    d = dict(dtype=dtype)
    for k, s in (("y", 2.0), ("res", 1.0), ("g", 1.0)):
        d[k] = (torch.randn(NT_ELEMS, device=DEV) * s).to(dtype)
    d["mask"] = torch.randint(0, 256, (NT_ELEMS // 8,), device=DEV, dtype=torch.uint8)
    yield d
    d.clear()
    torch.cuda.empty_cache()


def test_bn_apply_nontemporal(nt):
    """The 64 MiB threshold: bf16 (16411, 2048) resmode 2 with mask (67.2 MB, hoisted coefficients), fp16
    (174767, 192) resmode 1 with mask (64 MiB + 1.6 KB, nontemporal together with per-vector coefficients)."""
    dtype = nt["dtype"]
    rows, C = NT_ROWS_C[dtype]
    n = rows * C
    assert n * 2 >= 64 << 20
    resmode = 2 if dtype == torch.bfloat16 else 1
    torch.manual_seed(5)
    coef, rcoef = _coef4(C), _coef4(C)[:2 * C].contiguous()
    _run_apply(nt["y"][:n], nt["res"][:n], coef, rcoef, C, resmode, True, True, dtype, f"bn_apply NT {dtype}")


def test_bn_apply_unsupported_variant_raises():
    """A (resmode, relu, mask) combination outside the dispatched set is an error, not a silent no-op."""
    C = 8
    y, res = _rand16(4, C, torch.bfloat16), _rand16(4, C, torch.bfloat16)
    coef = _coef4(C)
    out = torch.full_like(y, float("nan"))
    with pytest.raises(RuntimeError, match="unsupported variant"):
        _C().bn_apply(y, coef, res, coef, out, C, 3, True, None)
    y32, out32 = torch.randn(4, C, device=DEV), _nan(4, C)
    with pytest.raises(RuntimeError, match="unsupported variant"):
        _C().bn_apply32(y32, coef, y32, coef, out32, C, 3, True)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 1c
def _reduce_ref(g, bits, ys, coefs, C):
    """fp64 [C, 2 * nbr] sums and their magnitudes (sum |dz|, sum |dz * xhat|) from the kernel's own inputs."""
    rows = g.numel() // C
    K = 2 * len(ys)
    ref = torch.zeros(C, K, dtype=torch.float64, device=DEV)
    mag = torch.zeros(C, K, dtype=torch.float64, device=DEV)
    for sl in _row_chunks(rows, C):
        dz = g.view(rows, C)[sl].double()
        if bits is not None:
            dz = dz * bits[sl]
        for b, (y, coef) in enumerate(zip(ys, coefs)):
            c64 = coef.double()
            t = dz * ((y.view(rows, C)[sl].double() - c64[2 * C:3 * C]) * c64[3 * C:4 * C])
            ref[:, 2 * b] += dz.sum(0)
            mag[:, 2 * b] += dz.abs().sum(0)
            ref[:, 2 * b + 1] += t.sum(0)
            mag[:, 2 * b + 1] += t.abs().sum(0)
    return ref, mag


def _check_reduce(g, mask, ys, coefs, rows, C, blocks, name, family="1c"):
    C_ = _C()
    S, K = C_.stat_slots(), 2 * len(ys)
    slots = _nan(S * C * K, dtype=torch.float64)
    C_.bn_bwd_reduce(g, mask, ys[0], coefs[0], ys[1] if K == 4 else None, coefs[1] if K == 4 else None, slots,
                     blocks, rows, C)
    assert bool(torch.isfinite(slots).all()), f"{name}: slot entries left unwritten"
    sl3 = slots.view(S, C, K)
    for s in range(S):  # slot s owns the block partials [s*blocks/S, (s+1)*blocks/S)
        if s * blocks // S == (s + 1) * blocks // S:
            assert not bool(sl3[s].any()), f"{name}: slot {s} owns no block but is not zero"
    bits = _mask_bits(mask, C) if mask is not None else None
    ref, mag = _reduce_ref(g, bits, ys, coefs, C)
    rpi = 256 // (C // 8)
    n_chain = math.ceil(rows / (blocks * rpi)) + rpi
    got = sl3.sum(0)
    nm.assert_sum(got, ref, mag, n_chain, name, K, family=family)
    sums = _nan(C * K, dtype=torch.float64)
    C_.bn_slot_sum(slots, C, K, sums)  # layout [k * C + c]
    nm.assert_within(sums.view(K, C).t(), got, 64 * 2.0 ** -53 * sl3.abs().sum(0), f"{name}: bn_slot_sum", K,
                     family=family)
    return slots


REDUCE_SHAPES = [(3000, 8), (3000, 128), (40009, 64), (997, 192)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", REDUCE_SHAPES)
@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("nbr", [1, 2])
def test_bn_bwd_reduce(nbr, masked, shape, dtype):
    """sum dz and sum dz*xhat per branch against fp64: (3000, 8) has 256 row lanes per block, (3000, 128) 12 blocks
    (fewer than the 64 slots), (40009, 64) 79 blocks, (997, 192) 10 row lanes with 16 idle threads.  xhat is formed
    from the fp32 mean / invstd passed in; its two roundings and the product's are the bound's + 4."""
    rows, C = shape
    torch.manual_seed(rows + C + nbr)
    g, y1, y2 = _rand16(rows, C, dtype), _rand16(rows, C, dtype, 1.5), _rand16(rows, C, dtype, 0.7)
    mask = torch.randint(0, 256, (rows * C // 8,), device=DEV, dtype=torch.uint8) if masked else None
    c1, c2 = _coef4(C, tiny=False), _coef4(C, tiny=False)
    blocks = _C().bn_bwd_reduce_blocks(rows, C)
    _check_reduce(g, mask, [y1, y2][:nbr], [c1, c2][:nbr], rows, C, blocks, f"bn_bwd_reduce {shape} {dtype} nbr={nbr}")


@pytest.mark.parametrize("blocks", [1, 3])
@pytest.mark.parametrize("dtype", DTYPES)
def test_bn_bwd_reduce_caller_chosen_blocks(dtype, blocks):
    rows, C = 3000, 128
    torch.manual_seed(blocks)
    g, y1, y2 = _rand16(rows, C, dtype), _rand16(rows, C, dtype, 1.5), _rand16(rows, C, dtype, 0.7)
    mask = torch.randint(0, 256, (rows * C // 8,), device=DEV, dtype=torch.uint8)
    _check_reduce(g, mask, [y1, y2], [_coef4(C, tiny=False), _coef4(C, tiny=False)], rows, C, blocks,
                  f"bn_bwd_reduce blocks={blocks} {dtype}")


def test_bn_bwd_reduce_block_cap(nt):
    """(16411, 2048): one row per block iteration, 1026 blocks wanted, capped to 1024: blocks 0 and 1 take a second
    row.  Masked with two branches and unmasked with one, on the shared 64 MiB tensors."""
    rows, C = 16411, 2048
    blocks = _C().bn_bwd_reduce_blocks(rows, C)
    assert blocks == 1024 and (rows + 15) // 16 == 1026
    torch.manual_seed(9)
    c1, c2 = _coef4(C, tiny=False), _coef4(C, tiny=False)
    _check_reduce(nt["g"], nt["mask"], [nt["y"], nt["res"]], [c1, c2], rows, C, blocks, f"reduce cap nbr=2 {nt['dtype']}")
    _check_reduce(nt["g"], None, [nt["y"]], [c1], rows, C, blocks, f"reduce cap nbr=1 {nt['dtype']}")


# ------------------------------------------------------------------------------------------------ 1d
@pytest.mark.parametrize("with_grads", [True, False])
@pytest.mark.parametrize("gscale", [1.0, 2.0 ** -19])
@pytest.mark.parametrize("C", [8, 200, 2048])
@pytest.mark.parametrize("K", [2, 4])
def test_bn_bwd_finalize(K, C, gscale, with_grads):
    """bn_bwd_finalize_slots (one launch, K = 2 or 4) and bn_slot_sum + bn_bwd_finalize per branch against the fp64
    formula from the fp64 slot sums and the fp32 coefficients passed in; bounds: check_bwd_finalize.  Buffers not
    passed (dgamma / dbeta = None) are simply not written; bcoef always is."""
    torch.manual_seed(K * 1000 + C)
    C_ = _C()
    S, count = C_.stat_slots(), 3001.0
    slots = torch.randn(S, C, K, dtype=torch.float64, device=DEV) * 5
    coefs = [_coef4(C, tiny=False) for _ in range(K // 2)]
    gammas = [(torch.rand(C, device=DEV) + 0.5) * _signs(C) for _ in range(K // 2)]
    tot = slots.sum(0)
    refs = [nm.bn_bwd_finalize_ref(tot[:, 2 * b], tot[:, 2 * b + 1], count, coefs[b], gammas[b], gscale, C)
            for b in range(K // 2)]
    mk = lambda: (_nan(C), _nan(C)) if with_grads else (None, None)
    # one launch
    dg, db, bc = [], [], []
    for b in range(K // 2):
        a, c = mk()
        dg.append(a), db.append(c), bc.append(_nan(3 * C))
    two = K == 4
    C_.bn_bwd_finalize_slots(slots, K, count, coefs[0], gammas[0], dg[0], db[0], bc[0], coefs[1] if two else None,
                             gammas[1] if two else None, dg[1] if two else None, db[1] if two else None,
                             bc[1] if two else None, gscale)
    for b in range(K // 2):
        nm.check_bwd_finalize(bc[b], dg[b], db[b], refs[b], C, f"bwd_finalize_slots K={K} C={C} branch {b}", family="1d")
    # two launches per branch
    sums = _nan(C * K, dtype=torch.float64)
    C_.bn_slot_sum(slots, C, K, sums)
    for b in range(K // 2):
        a, c = mk()
        bc2 = _nan(3 * C)
        C_.bn_bwd_finalize(sums[2 * b * C:(2 * b + 2) * C].contiguous(), count, coefs[b], gammas[b], a, c, gscale, bc2)
        nm.check_bwd_finalize(bc2, a, c, refs[b], C, f"bn_bwd_finalize K={K} C={C} branch {b}", family="1d")


# ------------------------------------------------------------------------------------------------ 1e
BWD_APPLY_VARIANTS = [(True, 1, False), (True, 1, True), (True, 2, False), (False, 1, False), (False, 2, False),
                      (False, 1, True)]


def _run_bwd_apply(g, mask, y1, y2, b1, b2, C, variant, dtype, name, family="1e"):
    masked, nbr, wdz = variant
    rows = g.numel() // C
    dy1 = torch.full_like(g, float("nan"))
    dy2 = torch.full_like(g, float("nan")) if nbr == 2 else None
    dz = torch.full_like(g, float("nan")) if wdz else None
    m = mask if masked else None
    _C().bn_bwd_apply(g, m, y1, b1, dy1, y2 if nbr == 2 else None, b2 if nbr == 2 else None, dy2, dz, C)
    g2 = g.view(rows, C)
    for sl in _row_chunks(rows, C):
        bits = _mask_bits(m.view(rows, C // 8)[sl], C) if masked else None
        dz16 = torch.where(bits, g2[sl], torch.zeros_like(g2[sl])) if masked else g2[sl]
        if wdz:  # bitwise g where the mask bit is set, +0 elsewhere
            assert torch.equal(dz.view(rows, C)[sl].view(torch.int16), dz16.view(torch.int16)), f"{name}: dz"
        for y, b, dy in ((y1, b1, dy1), (y2, b2, dy2))[:nbr]:
            ref, mag = nm.bn_bwd_apply_ref(dz16.double(), y.view(rows, C)[sl], b, C)
            nm.assert_rounded(dy.view(rows, C)[sl], ref, mag, dtype, name=f"{name} rows {sl.start}..", C=C, family=family)
    return dy1, dy2


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", APPLY_SHAPES)
@pytest.mark.parametrize("variant", BWD_APPLY_VARIANTS)
def test_bn_bwd_apply(variant, shape, dtype):
    """dy_b = A_b*dz + B_b*y_b + C_b rounded to 16 bits, dz = g under the mask: assert_rounded with
    mag = |A*dz| + |B*y| + |C|; dz written is bitwise g or +0."""
    rows, C = shape
    torch.manual_seed(rows * 3 + C)
    g, y1, y2 = _rand16(rows, C, dtype), _rand16(rows, C, dtype, 1.5), _rand16(rows, C, dtype, 0.7)
    mask = torch.randint(0, 256, (rows * C // 8,), device=DEV, dtype=torch.uint8)
    _run_bwd_apply(g, mask, y1, y2, _bcoef(C), _bcoef(C), C, variant, dtype, f"bn_bwd_apply{variant} {shape} {dtype}")


@pytest.mark.parametrize("variant", BWD_APPLY_VARIANTS)
def test_bn_bwd_apply_nontemporal(nt, variant):
    dtype = nt["dtype"]
    rows, C = NT_ROWS_C[dtype]
    n = rows * C
    torch.manual_seed(6)
    _run_bwd_apply(nt["g"][:n], nt["mask"][:n // 8], nt["y"][:n], nt["res"][:n], _bcoef(C), _bcoef(C), C, variant, dtype,
                   f"bn_bwd_apply NT {variant} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("masked", [True, False])
def test_bn_bwd_apply_two_branches_with_dz_is_not_dispatched(masked, dtype):
    """(mask, 2 branches, dz written) has no kernel: the launcher throws on the host before any launch."""
    rows, C = 16, 64
    g, y1, y2 = _rand16(rows, C, dtype), _rand16(rows, C, dtype), _rand16(rows, C, dtype)
    mask = torch.full((rows * C // 8,), 0xFF, dtype=torch.uint8, device=DEV) if masked else None
    dy1, dy2, dz = torch.full_like(g, float("nan")), torch.full_like(g, float("nan")), torch.full_like(g, float("nan"))
    with pytest.raises(RuntimeError, match="unsupported variant"):
        _C().bn_bwd_apply(g, mask, y1, _bcoef(C), dy1, y2, _bcoef(C), dy2, dz, C)
    torch.cuda.synchronize()
    assert bool(torch.isnan(dy1.float()).all() and torch.isnan(dz.float()).all())  # nothing ran


# ------------------------------------------------------------------------------------------------ 1f
@pytest.mark.parametrize("dtype", DTYPES)
def test_chain_in_executor_order(dtype):
    """relu(bn1(y1) + bn2(y2)) forward and backward through the kernels in the executor's order on (517, 64), every
    stage against fp64 from that stage's actual inputs, and dgamma / dbeta of both branches against torch.autograd in
    fp64 with the ReLU replaced by the kernel's mask.

    Bound of dgamma against autograd: the reduce bound (n_chain + 4) * u * sum|dz*xhat| (the + 4 holds the three
    roundings of dz * (y - mean) * invstd and the rounding of invstd to fp32), plus the rounding of mean to fp32 --
    xhat moves by at most u|mean|*invstd, doubled for the fp64 -> fp32 -> product path: 4u * sum|dz| * |mean*invstd| --
    plus the 2u|ref| of the finalize's fp32 result.  dbeta = sum dz does not see the coefficients: the reduce bound on
    sum|dz| plus 2u|ref|."""
    torch.manual_seed(31)
    C_ = _C()
    rows, C = 517, 64
    S = C_.stat_slots()
    ys = [(torch.randn(rows, C, device=DEV) * (torch.rand(C, device=DEV) * 2 + 0.2) + torch.randn(C, device=DEV)).to(dtype)
          for _ in range(2)]
    gammas = [(torch.rand(C, device=DEV) + 0.5) * _signs(C) for _ in range(2)]
    betas = [torch.randn(C, device=DEV) * 0.5 for _ in range(2)]
    coefs = []
    for b in range(2):  # 1. slots -> bn_finalize_slots
        y64 = ys[b].double()
        slots = _slots_from_rows(y64)
        rm0, rv0 = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
        rm, rv = rm0.clone(), rv0.clone()
        coef, sums = _nan(4 * C), _nan(2 * C, dtype=torch.float64)
        C_.bn_finalize_slots(slots, float(rows), gammas[b], betas[b], EPS, MOM, rm, rv, coef, sums, True)
        ref = nm.bn_finalize_ref(y64.sum(0), (y64 * y64).sum(0), float(rows), gammas[b], betas[b], EPS, MOM, rm0, rv0,
                                 var=y64.var(0, unbiased=False))
        nm.check_finalize(coef, rm, rv, ref, C, f"chain finalize branch {b}", family="1f")
        coefs.append(coef)
    # 2. bn_apply with mask
    out, mask = _run_apply(ys[0], ys[1], coefs[0], coefs[1][:2 * C].contiguous(), C, 2, True, True, dtype, "chain apply")
    # 3. bn_bwd_reduce
    g = _rand16(rows, C, dtype)
    blocks = C_.bn_bwd_reduce_blocks(rows, C)
    slots = _check_reduce(g, mask, ys, coefs, rows, C, blocks, "chain reduce", family="1f")
    # 4. bn_bwd_finalize_slots, K = 4
    dg, db, bc = [_nan(C), _nan(C)], [_nan(C), _nan(C)], [_nan(3 * C), _nan(3 * C)]
    C_.bn_bwd_finalize_slots(slots, 4, float(rows), coefs[0], gammas[0], dg[0], db[0], bc[0], coefs[1], gammas[1], dg[1],
                             db[1], bc[1], 1.0)
    tot = slots.view(S, C, 4).sum(0)
    for b in range(2):
        ref = nm.bn_bwd_finalize_ref(tot[:, 2 * b], tot[:, 2 * b + 1], float(rows), coefs[b], gammas[b], 1.0, C)
        nm.check_bwd_finalize(bc[b], dg[b], db[b], ref, C, f"chain bwd finalize branch {b}", family="1f")
    # 5. bn_bwd_apply
    _run_bwd_apply(g, mask, ys[0], ys[1], bc[0], bc[1], C, (True, 2, False), dtype, "chain bwd apply", family="1f")
    # autograd in fp64 with the kernel's mask as the ReLU
    bits = _mask_bits(mask, C).double()
    eps32 = float(torch.tensor(EPS).float())
    y64 = [y.double().requires_grad_(True) for y in ys]
    g64 = [x.double().requires_grad_(True) for x in gammas]
    b64 = [x.double().requires_grad_(True) for x in betas]
    pre = sum(F.batch_norm(y64[b], None, None, g64[b], b64[b], True, 0.1, eps32) for b in range(2))
    pre.backward(g.double() * bits)
    dz = g.double() * bits
    rpi = 256 // (C // 8)
    n_chain = math.ceil(rows / (blocks * rpi)) + rpi
    for b in range(2):
        yd = ys[b].double()
        mean = yd.mean(0)
        invstd = 1.0 / torch.sqrt(yd.var(0, unbiased=False) + eps32)
        xh = (yd - mean) * invstd
        gref, bref = g64[b].grad, b64[b].grad
        bound_g = (n_chain + 4) * U * (dz * xh).abs().sum(0) + 4 * U * dz.abs().sum(0) * (mean * invstd).abs() \
            + 2 * U * gref.abs()
        bound_b = (n_chain + 4) * U * dz.abs().sum(0) + 2 * U * bref.abs()
        nm.assert_within(dg[b], gref, bound_g, f"chain dgamma vs autograd, branch {b}", C, family="1f")
        nm.assert_within(db[b], bref, bound_b, f"chain dbeta vs autograd, branch {b}", C, family="1f")


# ------------------------------------------------------------------------------------------------ 1g
# C = 2048 makes n / 4 = rows * 512 a multiple of 256 for every row count; the other widths end in a partial block
F32_SHAPES = [(1031, 4), (77, 64), (37, 192), (5, 2048)]
# 16,780,800 elements: 4,195,200 float4 against the 16384 * 256 of one grid pass; the second pass steps the channel by
# (16384 * 256 * 4) % 192 = 64, which wraps past C for the threads that start at channel >= 128
F32_WRAP = (87400, 192)


def _run_apply32(rows, C, resmode, relu, name):
    y, res = torch.randn(rows, C, device=DEV) * 2, torch.randn(rows, C, device=DEV)
    coef, rcoef = _coef4(C), _coef4(C)[:2 * C].contiguous()
    out = _nan(rows, C)
    _C().bn_apply32(y, coef, res if resmode else None, rcoef if resmode == 2 else None, out, C, resmode, relu)
    for sl in _row_chunks(rows, C):
        _, ref, mag = nm.bn_apply_ref(y[sl], coef, res[sl], rcoef, C, resmode, relu)
        nm.assert_rounded(out[sl], ref, mag, torch.float32, name=f"{name} rows {sl.start}..", C=C, family="1g")


@pytest.mark.parametrize("shape", F32_SHAPES)
@pytest.mark.parametrize("resmode", [0, 1, 2])
@pytest.mark.parametrize("relu", [True, False])
def test_bn_apply32(relu, resmode, shape):
    rows, C = shape
    torch.manual_seed(rows + C + resmode)
    _run_apply32(rows, C, resmode, relu, f"bn_apply32 resmode={resmode} relu={relu} {shape}")


def test_bn_apply32_second_grid_pass_wraps_the_channel():
    torch.manual_seed(8)
    assert F32_WRAP[0] * F32_WRAP[1] // 4 > 16384 * 256 and (16384 * 256 * 4) % F32_WRAP[1] != 0
    _run_apply32(*F32_WRAP, 2, True, "bn_apply32 wrap")


def _run_bwd_apply32(rows, C, variant, name):
    masked, nbr, wdz = variant
    g, y1, y2 = torch.randn(rows, C, device=DEV), torch.randn(rows, C, device=DEV) * 1.5, torch.randn(rows, C, device=DEV)
    mref = torch.relu(torch.randn(rows, C, device=DEV)) if masked else None
    b1, b2 = _bcoef(C), _bcoef(C)
    dy1 = _nan(rows, C)
    dy2 = _nan(rows, C) if nbr == 2 else None
    dz = _nan(rows, C) if wdz else None
    _C().bn_bwd_apply32(g, mref, y1, b1, dy1, y2 if nbr == 2 else None, b2 if nbr == 2 else None, dy2, dz, C)
    for sl in _row_chunks(rows, C):
        dzr = torch.where(mref[sl] > 0, g[sl], torch.zeros_like(g[sl])) if masked else g[sl]
        if wdz:
            assert torch.equal(dz[sl].view(torch.int32), dzr.view(torch.int32)), f"{name}: dz"
        for y, b, dy in ((y1, b1, dy1), (y2, b2, dy2))[:nbr]:
            ref, mag = nm.bn_bwd_apply_ref(dzr.double(), y[sl], b, C)
            nm.assert_rounded(dy[sl], ref, mag, torch.float32, name=f"{name} rows {sl.start}..", C=C, family="1g")


BWD32_VARIANTS = [(m, n, z) for m in (True, False) for n in (1, 2) for z in (False, True)]


@pytest.mark.parametrize("shape", F32_SHAPES)
@pytest.mark.parametrize("variant", BWD32_VARIANTS)
def test_bn_bwd_apply32(variant, shape):
    rows, C = shape
    torch.manual_seed(rows + C)
    _run_bwd_apply32(rows, C, variant, f"bn_bwd_apply32{variant} {shape}")


def test_bn_bwd_apply32_second_grid_pass_wraps_the_channel():
    torch.manual_seed(9)
    _run_bwd_apply32(*F32_WRAP, (True, 2, False), "bn_bwd_apply32 wrap")


@pytest.mark.parametrize("shape", [(3000, 4), (2000, 64), (997, 192), (300, 1024), (300, 2048)])
@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("nbr", [1, 2])
def test_bn_bwd_reduce32(nbr, masked, shape):
    """The fp32 reduce (dz = g where the post-ReLU reference is > 0): C = 192 has 5 row lanes of 48 threads, 1024 one
    row per iteration, 2048 two float4 groups per thread (NV = 2).  Same chain bound as the 16-bit reduce."""
    rows, C = shape
    torch.manual_seed(rows + C + nbr)
    C_ = _C()
    S, K = C_.stat_slots(), 2 * nbr
    g = torch.randn(rows, C, device=DEV)
    ys = [torch.randn(rows, C, device=DEV) * 1.5, torch.randn(rows, C, device=DEV) * 0.7][:nbr]
    coefs = [_coef4(C, tiny=False), _coef4(C, tiny=False)][:nbr]
    mref = torch.relu(torch.randn(rows, C, device=DEV)) if masked else None
    blocks = C_.bn_bwd_reduce32_blocks(rows, C)
    slots = _nan(S * C * K, dtype=torch.float64)
    C_.bn_bwd_reduce32(g, mref, ys[0], coefs[0], ys[1] if nbr == 2 else None, coefs[1] if nbr == 2 else None, slots,
                       blocks, rows, C)
    assert bool(torch.isfinite(slots).all())
    ref, mag = _reduce_ref(g, (mref > 0) if masked else None, ys, coefs, C)
    vpr = C // 4
    nv = vpr // 256 if vpr > 256 else 1
    rpi = 256 // (vpr // nv)
    n_chain = math.ceil(rows / (blocks * rpi)) + rpi
    nm.assert_sum(slots.view(S, C, K).sum(0), ref, mag, n_chain, f"bn_bwd_reduce32 {shape} nbr={nbr}", K, family="1g")


def test_bn_bwd_reduce32_rejects_an_unsupported_width():
    rows, C = 4, 1536
    g = torch.randn(rows, C, device=DEV)
    slots = _nan(_C().stat_slots() * C * 2, dtype=torch.float64)
    with pytest.raises(RuntimeError):
        _C().bn_bwd_reduce32(g, None, g, _coef4(C), None, None, slots, 1, rows, C)
    torch.cuda.synchronize()


@pytest.mark.parametrize("N,H,W,C", [(2, 12, 11, 64), (2, 13, 11, 64), (3, 27, 27, 192), (2, 55, 55, 64)])
def test_maxpool_bwd_relu32(N, H, W, C):
    """Gather-form backward of MaxPool(3, 2, 1) with the ReLU mask recomputed from y, against a plain fp64 scatter of the
    pooled gradient along the argmax bytes (the sizes of the 16-bit pool test).  A pixel collects at most 4 window
    gradients in fp32: assert_sum with a chain of 4; elements whose BN value is within its own 8u bound of 0 (the ReLU
    decision could go either way) are not compared."""
    torch.manual_seed(H * W)
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    y = torch.randn(N, H, W, C, device=DEV)
    coef = _coef4(C, tiny=False)
    dp = torch.randn(N, OH, OW, C, device=DEV)
    idx = torch.randint(0, 9, (N, OH, OW, C), device=DEV, dtype=torch.uint8)
    dz = _nan(N, H, W, C)
    _C().maxpool_bwd_relu32(dp, idx, y, coef, dz, N, H, W, C)
    ref = torch.zeros(N, H, W, C, dtype=torch.float64, device=DEV)
    mag = torch.zeros_like(ref)
    n_i, oh_i, ow_i, c_i = torch.meshgrid(*[torch.arange(s, device=DEV) for s in (N, OH, OW, C)], indexing="ij")
    h = oh_i * 2 - 1 + (idx // 3).long()
    w = ow_i * 2 - 1 + (idx % 3).long()
    ok = (h >= 0) & (h < H) & (w >= 0) & (w < W)
    flat = ((n_i * H + h) * W + w) * C + c_i
    ref.view(-1).index_put_((flat[ok],), dp.double()[ok], accumulate=True)
    mag.view(-1).index_put_((flat[ok],), dp.double().abs()[ok], accumulate=True)
    c64 = coef.double()
    t1, t2 = y.double() * c64[:C], c64[C:2 * C]
    val = t1 + t2
    ref = torch.where(val > 0, ref, torch.zeros_like(ref))
    sure = val.abs() > 8 * U * (t1.abs() + t2.abs())
    assert bool(torch.isfinite(dz).all())
    nm.assert_sum(dz[sure], ref[sure], mag[sure], 4, "maxpool_bwd_relu32", family="1g")


# ------------------------------------------------------------------------------------------------ 1h: the fp32 stem tail
import _conv_cases as cc  # noqa: E402


def _pool_windows(v_nhwc, fill):
    """[N, H, W, C] fp64 -> [N, OH, OW, C, 9]: the 3x3 / stride 2 / pad 1 windows, positions outside the image = fill."""
    N, H, W, C = v_nhwc.shape
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    p = F.pad(v_nhwc.permute(0, 3, 1, 2), (1, 1, 1, 1), value=fill)
    cols = F.unfold(p, (3, 3), stride=2).view(N, C, 9, OH, OW)
    return cols.permute(0, 3, 4, 1, 2).contiguous()


@pytest.mark.parametrize("N,H,W,C", [(2, 12, 11, 64), (2, 13, 11, 64), (3, 27, 27, 192), (2, 55, 55, 64), (2, 13, 11, 4)])
def test_bn_relu_maxpool32(N, H, W, C):
    """out within 8u * mag of the fp64 max(relu(y * scale + shift)) over the in-image window (mag: the largest
    |y * scale| + |shift| of the window: the maximum of values each off by at most that is off by at most that); idx
    names an in-image window position whose fp64 value is within the bound of the maximum (near-ties may go either
    way).  Odd H / W: border windows of 4 and 6 members."""
    torch.manual_seed(H * W + C)
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    y = torch.randn(N, H, W, C, device=DEV)
    coef = _coef4(C, tiny=False)
    out, idx = _nan(N, OH, OW, C), torch.full((N, OH, OW, C), 255, dtype=torch.uint8, device=DEV)
    _C().bn_relu_maxpool32(y, coef, out, idx, N, H, W, C)
    c64 = coef.double()
    t1, t2 = y.double() * c64[:C], c64[C:2 * C]
    win = _pool_windows(torch.relu(t1 + t2), -1.0)
    bound = 8 * U * _pool_windows(t1.abs() + t2.abs().expand_as(t1), 0.0).max(-1).values
    ref = win.max(-1).values
    nm.assert_within(out, ref, bound, "bn_relu_maxpool32: out", C, family="1h", shape=ref.shape)
    assert bool((idx < 9).all()), "bn_relu_maxpool32: an argmax byte was not written or is not a window position"
    chosen = win.gather(-1, idx.long().unsqueeze(-1)).squeeze(-1)
    assert bool((chosen >= 0).all()), "bn_relu_maxpool32: idx names a position outside the image"
    nm.assert_within(chosen, ref, bound, "bn_relu_maxpool32: value at idx", C, shape=ref.shape)


@pytest.mark.parametrize("N,H,W,C", [(2, 13, 11, 64), (3, 9, 7, 4)])
def test_bn_relu_maxpool32_decisive(N, H, W, C):
    """Integer y whose 9 values differ inside every 3x3 window (a per-plane permutation of -4 .. 4 laid out by (h % 3,
    w % 3)), power-of-two scale, shift 0.5: every window value is exact, a positive maximum is unique, and negative
    values all clamp to 0 -- an all-negative window (planes c % 8 == 5 hold -9 .. -1 under a positive scale) gives
    out == 0 at the first in-image position.  out and idx must match exactly."""
    g = torch.Generator().manual_seed(H + C)
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    perm = (torch.argsort(torch.rand(N, C, 9, generator=g), dim=-1) - 4).float()
    ch = torch.arange(C)
    perm[:, ch % 8 == 5] -= 5.0
    pos = (torch.arange(H).view(H, 1) % 3) * 3 + torch.arange(W).view(1, W) % 3
    y = perm[:, :, pos].permute(0, 2, 3, 1).contiguous().to(DEV)
    scale = torch.tensor([1.0, 2.0, 4.0])[ch % 3] * torch.where((ch // 3) % 2 == 0, 1.0, -1.0)
    scale[ch % 8 == 5] = 2.0
    coef = torch.cat([scale, torch.full((C,), 0.5), torch.zeros(2 * C)]).to(DEV)
    out, idx = _nan(N, OH, OW, C), torch.full((N, OH, OW, C), 255, dtype=torch.uint8, device=DEV)
    _C().bn_relu_maxpool32(y, coef, out, idx, N, H, W, C)
    win = _pool_windows(torch.relu(y.double() * coef[:C].double() + 0.5), -1.0)
    ref = win.max(-1)
    assert bool((ref.values[..., ch % 8 == 5] == 0).all()) and bool((ref.values > 0).any())
    nm.assert_within(out, ref.values, 0.0, "bn_relu_maxpool32 decisive: out", C, shape=ref.values.shape)
    bad = (idx.long() != ref.indices).nonzero()
    assert bad.numel() == 0, (f"bn_relu_maxpool32 decisive: {bad.shape[0]} argmax bytes differ; first at (n, oh, ow, c) = "
                              f"{tuple(bad[0].tolist())}: got {int(idx[tuple(bad[0])])}, "
                              f"expected {int(ref.indices[tuple(bad[0])])}")


@pytest.mark.parametrize("N,H,W,C", [(2, 12, 11, 64), (2, 13, 11, 64), (2, 55, 55, 64), (2, 13, 11, 4)])
def test_stem_pool_bwd_apply32(N, H, W, C):
    """dy = A*dz + B*y + Cc with dz recomputed in the kernel, against the fp64 scatter + mask of cc.stem_tail_ref and
    nm.bn_bwd_apply_ref's formula: (8 + 4) * u * mag -- the elementwise budget plus the up to 4 window gradients dz
    collects in fp32.  Elements whose ReLU sign fp32 may call either way are not compared.  C = 4: cshift = 0."""
    d = {k: v.to(DEV).contiguous() for k, v in cc.stem32_tail_operands(N, H, W, "real", C=C).items()}
    r = cc.stem_tail_ref(d, N, H, W, C)
    ref, mag = nm.bn_bwd_apply_ref(r["dz"], d["y"], d["b"], C)
    assert float((ref.view_as(r["dy"]) - r["dy"]).abs().max()) == 0.0
    dy = _nan(N, H, W, C)
    _C().stem_pool_bwd_apply32(d["dp"].view(-1), d["idx"].view(-1), d["y"].view(-1), d["coef"], d["b"], dy.view(-1), N, H,
                               W, C)
    assert bool(torch.isfinite(dy).all())
    sure = ~r["unsure"]
    assert float(sure.double().mean()) > 0.99
    nm.assert_within(dy[sure], r["dy"][sure], 12 * U * r["dymag"][sure], "stem_pool_bwd_apply32", family="1h")


@pytest.mark.parametrize("N,H,W,C,blocks", [(2, 13, 11, 64, 1), (2, 13, 11, 64, 7), (2, 12, 11, 64, 7), (1, 3, 5, 64, 20),
                                            (2, 13, 11, 4, 7)])
def test_stem_pool_bwd_reduce32(N, H, W, C, blocks):
    """sum dz and sum dz * xhat against the same fp64 dz: the chain bound of the kernel's lane plan (rpi = 256 / (C / 4)
    row lanes, as test_bn_bwd_reduce32) with 4 more additions for the window gradients dz collects; a pixel whose ReLU
    sign fp32 may call either way may contribute its gradient or nothing.  blocks = 20 exceeds the 15 pixel rows."""
    C_ = _C()
    S = C_.stat_slots()
    d = {k: v.to(DEV).contiguous() for k, v in cc.stem32_tail_operands(N, H, W, "real", C=C, seed=blocks).items()}
    r = cc.stem_tail_ref(d, N, H, W, C)
    rows = N * H * W
    slots = _nan(S * C * 2, dtype=torch.float64)
    C_.reset_dispatch_counts()
    C_.stem_pool_bwd_reduce32(d["dp"].view(-1), d["idx"].view(-1), d["y"].view(-1), d["coef"], slots, blocks, N, H, W, C)
    torch.cuda.synchronize()
    assert dict(C_.dispatch_counts()).get("stem_pool_bwd_fused32", 0) == 1
    assert bool(torch.isfinite(slots).all())
    got = slots.view(S, C, 2).sum(0)
    xh = nm.bn_xhat(d["y"], d["coef"], C)
    dz, dzmag = r["dz"].reshape(-1, C), r["dzmag"].reshape(-1, C)
    flip = torch.where(r["unsure"].reshape(-1, C), dzmag, torch.zeros_like(dzmag))
    rpi = 256 // (C // 4)
    n_chain = math.ceil(rows / (blocks * rpi)) + rpi + 4
    ref = torch.stack([dz.sum(0), (dz * xh).sum(0)], 1)
    mag = torch.stack([dzmag.sum(0), (dzmag * xh.abs()).sum(0)], 1)
    extra = torch.stack([flip.sum(0), (flip * xh.abs()).sum(0)], 1)
    nm.assert_within(got, ref, (n_chain + 4) * U * mag + extra, f"stem_pool_bwd_reduce32 blocks={blocks}", 2, family="1h")


@pytest.mark.parametrize("Cin", [1, 3])
@pytest.mark.parametrize("N,H,W,extra", [(2, 9, 7, 0), (3, 32, 24, 2), (1, 5, 6, 5)])
def test_stem_pack32(N, H, W, extra, Cin):
    """The zero-padded NHWC4 image equals the NCHW input bit for bit at every interior pixel and is exactly zero in
    the unused channels, in the border and in the extra rows and columns (Hp, Wp larger than H + 2 * pad)."""
    torch.manual_seed(H + W + Cin)
    pad = 3
    Hp, Wp = H + 2 * pad + extra, W + 2 * pad + (extra + 1 if extra else 0)
    x = torch.randn(N, Cin, H, W, device=DEV)
    x[0, 0, 0, 0] = -0.0
    out = _nan(N, Hp, Wp, 4)
    _C().stem_pack32(x, out.view(-1), N, Cin, H, W, pad, Hp, Wp)
    expect = torch.zeros(N, Hp, Wp, 4, device=DEV)
    expect[:, pad:pad + H, pad:pad + W, :Cin] = x.permute(0, 2, 3, 1)
    bad = (out.view(torch.int32) != expect.view(torch.int32)).nonzero()
    assert bad.numel() == 0, (f"stem_pack32: {bad.shape[0]} elements differ; first at (n, hp, wp, c) = "
                              f"{tuple(bad[0].tolist())}: got {float(out[tuple(bad[0])])!r}, "
                              f"expected {float(expect[tuple(bad[0])])!r}")
