"""The small loss, pooling and layout kernels called directly, per element against fp64: xent / xent32, metrics,
colsum / colsum32, avgpool_fwd / avgpool_bwd / avgpool32_*, nhwc_nchw16, im2col / im2col32.

Bounds (u = 2**-24, tests/_numerics.py):

* xent row loss: 2**-18 * (1 + |max logit| + |loss|).  The kernel forms logit + bias in fp32 (u each), subtracts the
  maximum, and uses the fast __expf / __logf (a few ulp each on arguments up to a few tens, i.e. an absolute error of a
  few u times the argument in the exponent); the wave sum adds log2(64) + ncls/64 roundings.  64u of the magnitudes
  involved holds all of that; torch's own fp32 cross_entropy is asserted to stay inside the same bound.
* xent dlogits: half a 16-bit ulp at |ref| + 2**-18 * gs with gs = loss_scale / grad_div (softmax probabilities are
  at most 1, their relative error is the exponent's absolute error).
* metrics / colsum / colsum32: assert_sum with the kernel's chain length.
* avgpool forward: half a 16-bit ulp + (HW + 2) * u * sum|x| / HW (a chain of HW additions, the rounded 1 / HW and the
  product); backward: half a 16-bit ulp + 2u|ref|.
* layout kernels: exact.

Output buffers start as NaN or a sentinel; padding that must not be read is NaN, padding that must not be written keeps
its sentinel.

Worst observed error / bound on an MI355X with these seeds (information, not a threshold): xent 0.9997 (the 16-bit
dlogits, whose half-ulp term is tight by construction), metrics 0.08, colsum32 0.23, avgpool 0.994 (again the 16-bit
rounding); the layout kernels are exact.
"""
import math

import pytest
import torch
import torch.nn.functional as F

import _numerics as nm
from _numerics import U

pytestmark = pytest.mark.gpu

DEV = "cuda"
DT3 = [torch.bfloat16, torch.float16, torch.float32]
DT3_IDS = ["bf16", "fp16", "fp32"]

def _C():
    from pytorch_distributed_template_amd.ops import native
    return native.C


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


# ------------------------------------------------------------------------------------------------ xent
def _first_argmax(v):
    """index of the first maximum of each row"""
    n = v.shape[1]
    ar = torch.arange(n, device=v.device).expand_as(v)
    return torch.where(v == v.max(1, keepdim=True).values, ar, torch.full_like(ar, n)).min(1).values


def _run_xent(logits, ld, bias, tgt, B, ncls, dtype, loss_scale, grad_div, outputs, name):
    """Calls xent / xent32 and checks everything it wrote; logits is [B, ld] with NaN in the padding columns."""
    C_ = _C()
    out = _nan(B, ncls) if outputs else None
    d = _nan(B, ld, dtype=dtype) if outputs else None
    rl, rc = _nan(B), _nan(B)
    ls = torch.full((1,), loss_scale, device=DEV) if loss_scale is not None else None
    if dtype == torch.float32:
        C_.xent32(logits, ld, bias, tgt, B, ncls, out, d, ls, float(grad_div), rl, rc)
    else:
        C_.xent(logits, ld, bias, tgt, B, ncls, out, d, ls, float(grad_div), rl, rc)
    gs = (loss_scale if loss_scale is not None else 1.0) / grad_div
    r = nm.xent_ref(logits, bias, tgt, ncls, gs, dtype)  # shared with the step audit (tests/_step_audit.py)
    v64, loss, bound = r["v"], r["loss"], r["loss_bound"]
    nm.assert_within(rl, loss, bound, f"{name}: row loss", family="3 xent")
    # the bound is reachable: torch's fp32 cross entropy of the same values stays inside it
    nm.assert_within(F.cross_entropy(v64.float(), tgt, reduction="none"), loss, bound, f"{name}: torch fp32 loss")
    v32 = logits[:, :ncls].float() + (bias if bias is not None else 0.0)  # the fp32 values the kernel compares
    assert torch.equal(rc, (_first_argmax(v32) == tgt).float()), f"{name}: row_correct"
    assert torch.equal(r["correct"], (_first_argmax(v32) == tgt).float())
    if outputs:
        nm.assert_rounded(out, v64, r["vmag"], torch.float32, k=1, name=f"{name}: out_logits", C=ncls, family="3 xent")
        nm.assert_within(d[:, :ncls], r["dlogits"], r["dlogits_bound"], f"{name}: dlogits", ncls, family="3 xent")
        assert not bool(d[:, ncls:].float().ne(0).any()), f"{name}: dlogits padding columns must be zero"
    return rl, rc


def _logits(B, ncls, ld, dtype, scale=3.0):
    lg = _nan(B, ld, dtype=dtype)
    lg[:, :ncls] = (torch.randn(B, ncls, device=DEV) * scale).to(dtype)
    return lg


XENT_SHAPES = [(37, 1000, 1024), (5, 10, 16), (3, 64, 64), (9, 130, 136), (1, 1000, 1024)]


@pytest.mark.parametrize("dtype", DT3, ids=DT3_IDS)
@pytest.mark.parametrize("shape", XENT_SHAPES)
def test_xent_rows_against_fp64(shape, dtype):
    """Per-row loss, correctness flag, biased fp32 logits and the 16-bit (or fp32) backward seed, with a bias, a loss
    scale of 8 and grad_div = B; fewer than 64 classes leave lanes idle, 130 classes a partial third stride."""
    B, ncls, ld = shape
    torch.manual_seed(B + ncls)
    lg = _logits(B, ncls, ld, dtype)
    bias = torch.randn(ncls, device=DEV) * 0.1
    tgt = torch.randint(0, ncls, (B,), device=DEV)
    tgt[0] = int(_first_argmax(lg[:1, :ncls].float() + bias)[0])  # at least one correct row
    _run_xent(lg, ld, bias, tgt, B, ncls, dtype, 8.0, B, True, f"xent {shape} {dtype}")


@pytest.mark.parametrize("dtype", DT3, ids=DT3_IDS)
@pytest.mark.parametrize("option", ["no_bias", "no_loss_scale", "grad_div_4B", "eval", "pm60"])
def test_xent_options(option, dtype):
    B, ncls, ld = 9, 130, 136
    torch.manual_seed(len(option))
    lg = _logits(B, ncls, ld, dtype)
    bias = None if option == "no_bias" else torch.randn(ncls, device=DEV) * 0.1
    if option == "pm60":  # saturated logits: exp underflows to 0 for most classes, losses up to 120
        lg[:, :ncls] = torch.where(torch.rand(B, ncls, device=DEV) < 0.5, -60.0, 60.0).to(dtype)
    tgt = torch.randint(0, ncls, (B,), device=DEV)
    _run_xent(lg, ld, bias, tgt, B, ncls, dtype, None if option == "no_loss_scale" else 8.0,
              4 * B if option == "grad_div_4B" else B, option != "eval", f"xent {option} {dtype}")


@pytest.mark.parametrize("dtype", DT3, ids=DT3_IDS)
@pytest.mark.parametrize("ncls,ld,first,second", [(1000, 1024, 5, 69), (1000, 1024, 70, 200), (1000, 1024, 10, 65),
                                                  (1000, 1024, 63, 64), (10, 16, 2, 7)])
def test_xent_tie_for_the_maximum_counts_the_first_index(ncls, ld, first, second, dtype):
    """Two equal maxima: correct only when the target is the first of them -- in the same lane across two 64-column
    strides (5, 69), in different lanes and strides (70, 200), with the first maximum in the HIGHER lane (10 vs 65:
    lane 10 against lane 1, the wave reduction must compare indices, not lanes), adjacent across a stride boundary,
    and with fewer than 64 classes."""
    torch.manual_seed(first)
    B = 2
    lg = _logits(B, ncls, ld, dtype, scale=1.0)
    lg[:, first] = 6.0
    lg[:, second] = 6.0
    tgt = torch.tensor([first, second], device=DEV)
    _, rc = _run_xent(lg, ld, None, tgt, B, ncls, dtype, None, B, True, f"xent tie {first}/{second} {dtype}")
    assert rc.tolist() == [1.0, 0.0]


# ------------------------------------------------------------------------------------------------ metrics / colsum32
@pytest.mark.parametrize("B", [1, 257, 1200])
def test_metrics_mean(B):
    """[mean(row_loss), mean(row_correct)]: a thread adds ceil(B / 256) values, the wave reduction 6 more, then the 4
    wave partials; the division by B is inside the bound's + 4."""
    torch.manual_seed(B)
    rl = torch.rand(B, device=DEV) * 7
    rc = (torch.rand(B, device=DEV) < 0.3).float()
    out = _nan(2)
    _C().metrics(rl, rc, B, out)
    n_chain = math.ceil(B / 256) + 6 + 3
    ref = torch.stack([rl.double().mean(), rc.double().mean()])
    nm.assert_sum(out, ref, ref.abs(), n_chain, f"metrics B={B}", family="3 metrics")


@pytest.mark.parametrize("B,ld,ncols", [(1200, 1024, 1000), (37, 1024, 1000), (5, 130, 130), (64, 136, 128)])
def test_colsum32(B, ld, ncols):
    """out[c] = scale * sum_b d[b][c] in fp32: 4 row lanes of ceil(B / 4) additions, 3 to combine them, the product with
    scale inside the + 4.  Columns >= ncols are not read (NaN) and out beyond ncols is not written."""
    torch.manual_seed(B + ncols)
    scale = 0.37
    d = _nan(B, ld)
    d[:, :ncols] = torch.randn(B, ncols, device=DEV)
    out = torch.full((ncols + 3,), -7.5, device=DEV)
    _C().colsum32(d, B, ld, ncols, out, scale)
    s32 = float(torch.tensor(scale, dtype=torch.float32))
    d64 = d[:, :ncols].double()
    nm.assert_sum(out[:ncols], s32 * d64.sum(0), abs(s32) * d64.abs().sum(0), math.ceil(B / 4) + 3,
                  f"colsum32 {(B, ld, ncols)}", family="3 colsum32")
    assert bool((out[ncols:] == -7.5).all())


@pytest.mark.parametrize("dtype", DT3[:2], ids=DT3_IDS[:2])
@pytest.mark.parametrize("B,ld,ncols", [(1200, 1024, 1000), (37, 1024, 1000), (5, 130, 130), (64, 136, 128)])
def test_colsum16(B, ld, ncols, dtype):
    """The 16-bit colsum per element at test_colsum32's shapes: ncols % 8 == 0 and ld % 8 == 0 run the 16-byte kernel (32
    row lanes of ceil(B / 32) additions, 31 to combine them), (5, 130, 130) the scalar one (4 lanes, 3 to combine); the
    16-bit inputs are exact in fp32 and the output is fp32.  Columns >= ncols are not read (NaN), out beyond ncols is not
    written."""
    torch.manual_seed(B + ncols)
    scale = 0.37
    d = _nan(B, ld, dtype=dtype)
    d[:, :ncols] = torch.randn(B, ncols, device=DEV).to(dtype)
    d[:, 1] *= 1e-3  # a column of small magnitude cannot hide in a norm
    out = torch.full((ncols + 3,), -7.5, device=DEV)
    _C().colsum(d, B, ld, ncols, out, scale)
    s32 = float(torch.tensor(scale, dtype=torch.float32))
    d64 = d[:, :ncols].double()
    n_chain = math.ceil(B / 32) + 31 if ncols % 8 == 0 and ld % 8 == 0 else math.ceil(B / 4) + 3
    nm.assert_sum(out[:ncols], s32 * d64.sum(0), abs(s32) * d64.abs().sum(0), n_chain, f"colsum {(B, ld, ncols)} {dtype}",
                  family=f"3 colsum16 {str(dtype).split('.')[-1]}")
    assert bool((out[ncols:] == -7.5).all())


# ------------------------------------------------------------------------------------------------ avgpool
# the 16-bit kernels move 8 channels per thread: C = 4 is an fp32-only case
AVGPOOL_CASES = [(s, dt) for s in [(3, 49, 512, 512), (2, 1, 64, 72), (5, 36, 2048, 2048)] for dt in DT3] + \
    [((3, 49, 4, 12), torch.float32)]


@pytest.mark.parametrize("shape,dtype", AVGPOOL_CASES)
def test_avgpool_fwd_and_bwd(shape, dtype):
    """Global average pool [N][HW][C] -> feat[N][ldf] and its backward; feature columns [C, ldf) keep their sentinel,
    and the backward does not read them (NaN)."""
    N, HW, C, ldf = shape
    C_ = _C()
    torch.manual_seed(N * HW + C)
    x = (torch.randn(N, HW, C, device=DEV) * 2 + 0.5).to(dtype)
    feat = torch.full((N, ldf), 7.0, dtype=dtype, device=DEV)
    if dtype == torch.float32:
        C_.avgpool32_fwd(x, feat, N, HW, C, ldf)
    else:
        C_.avgpool_fwd(x, feat, N, HW, C, ldf)
    x64 = x.double()
    ref = x64.mean(1)
    bound = nm.half_ulp16(ref, dtype) + (HW + 2) * U * x64.abs().sum(1) / HW
    nm.assert_within(feat[:, :C], ref, bound, f"avgpool fwd {(N, HW, C, ldf)} {dtype}", C, family="3 avgpool")
    assert bool((feat[:, C:] == 7.0).all())
    dfeat = _nan(N, ldf, dtype=dtype)
    dfeat[:, :C] = torch.randn(N, C, device=DEV).to(dtype)
    g = _nan(N, HW, C, dtype=dtype)
    if dtype == torch.float32:
        C_.avgpool32_bwd(dfeat, g, N, HW, C, ldf)
    else:
        C_.avgpool_bwd(dfeat, g, N, HW, C, ldf)
    gref = (dfeat[:, :C].double() / HW).unsqueeze(1).expand(N, HW, C)
    nm.assert_within(g, gref, nm.half_ulp16(gref, dtype) + 2 * U * gref.abs(), f"avgpool bwd {(N, HW, C, ldf)} {dtype}",
                     C, family="3 avgpool")


# ------------------------------------------------------------------------------------------------ layout
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("N,HW,C", [(3, 49, 512), (2, 36, 24), (1, 1, 8)])
def test_nhwc_nchw16(N, HW, C, dtype):
    torch.manual_seed(HW + C)
    x = torch.randn(N, HW, C, device=DEV).to(dtype)
    nchw = _nan(N, C, HW, dtype=dtype)
    _C().nhwc_nchw16(x, nchw, N, HW, C, True)
    assert torch.equal(nchw.view(torch.int16), x.permute(0, 2, 1).contiguous().view(torch.int16))
    back = _nan(N, HW, C, dtype=dtype)
    _C().nhwc_nchw16(nchw, back, N, HW, C, False)
    assert torch.equal(back.view(torch.int16), x.view(torch.int16))
    y = torch.randn(N, C, HW, device=DEV).to(dtype)  # the other direction from an independent tensor
    nhwc = _nan(N, HW, C, dtype=dtype)
    _C().nhwc_nchw16(y, nhwc, N, HW, C, False)
    assert torch.equal(nhwc.view(torch.int16), y.permute(0, 2, 1).contiguous().view(torch.int16))


# (N, C, H, W, R, S, stride, pad, extra columns): the stem-pack test's image sizes under the 7x7/2 pad-3 stem (the C = 3,
# S = 7 specialisation of im2col32), and two other filters for the generic kernel
IM2COL_GEOMS = [(3, 3, 17, 224, 7, 7, 2, 3, 0), (2, 3, 9, 24, 7, 7, 2, 3, 2), (2, 3, 7, 20, 7, 7, 2, 3, 1),
                (1, 3, 5, 18, 7, 7, 2, 3, 2), (2, 5, 9, 11, 3, 3, 1, 1, 1), (2, 3, 23, 19, 11, 11, 4, 2, 0)]


@pytest.mark.parametrize("dtype", DT3, ids=DT3_IDS)
@pytest.mark.parametrize("geom", IM2COL_GEOMS)
def test_im2col_matches_unfold(geom, dtype):
    """NCHW fp32 images -> im2col rows [N*OH*OW][ldk], column (r*S + s)*C + c, zeros outside the image and in the
    padding columns: exactly F.unfold's values (rounded to 16 bits by im2col, untouched by im2col32)."""
    N, C, H, W, R, S, stride, pad, ex = geom
    torch.manual_seed(H * W)
    q = 4 if dtype == torch.float32 else 8
    KK = R * S * C
    ldk = (KK + q - 1) // q * q + q * ex
    OH, OW = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - S) // stride + 1
    x = torch.randn(N, C, H, W, device=DEV)
    out = _nan(N * OH * OW, ldk, dtype=dtype)
    if dtype == torch.float32:
        _C().im2col32(x, out, N, C, H, W, R, S, stride, pad, ldk)
    else:
        _C().im2col(x, out, N, C, H, W, R, S, stride, pad, ldk)
    cols = F.unfold(x, (R, S), padding=pad, stride=stride)  # [N, C*R*S, L], row c*(R*S) + r*S + s
    ref = torch.zeros(N * OH * OW, ldk, device=DEV)
    ref[:, :KK] = cols.view(N, C, R * S, OH * OW).permute(0, 3, 2, 1).reshape(N * OH * OW, KK)
    assert torch.equal(out, ref.to(dtype))
