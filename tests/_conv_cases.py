"""The conv cases and operands shared by tests/test_conv_numerics_gpu.py, tests/test_conv32_numerics_gpu.py (the
kernels; the fp32 path's lists are at the end) and tests/test_numerics_model_cpu.py (the error model): one list, so they
cannot drift apart (a plain module).

A geometry is ``(N, H, W, C, K, R, stride, pad)``: NHWC input [N, H, W, C], KRSC weight [K, R, R, C].  Operands are
made on the CPU generator and are the same numbers wherever they are used.

Layer A (``layer="int"``): activations, gradients and residuals from {-2, -1, 1, 2}, weights from {-1, 1}: no zeros,
so every dropped, doubled or misplaced term changes the integer result, and every partial sum is exact in fp32.
Layer B (``layer="real"``): randn rounded to the dtype, weights scaled by (reduction length)**-0.5; fp16 and fp32 cases
scale one output channel by 1e-3 (fp16 outputs approach the subnormal range; a small channel cannot hide in a norm).
"""
import torch

import _numerics as nm

DTYPES = [torch.bfloat16, torch.float16]
F32 = torch.float32
# layer B scales one output channel (and that channel of the residual) by 1e-3 for these dtypes: fp16 outputs approach
# the subnormal range, and an fp32 channel of small magnitude cannot hide in a norm
SMALL_CHANNEL = (torch.float16, torch.float32)
XVALS = (-2, -1, 1, 2)
WVALS = (-1, 1)

# every compiled tile of the generic 2-stage / 3-stage ring kernel (test_kernels_gpu.TILES) runs this one
TILE_GEOM = (2, 15, 13, 256, 256, 3, 2, 1)  # ragged M tail, odd map, four dgrad phases of unequal size
DEFAULT_GEOMS = [
    (2, 14, 14, 64, 64, 3, 1, 1),
    (2, 15, 13, 64, 128, 3, 2, 1),
    (3, 14, 14, 128, 256, 1, 2, 0),  # dgrad: three phases without taps
    (2, 12, 12, 64, 256, 1, 1, 0),   # one K-step
    (1, 9, 9, 128, 128, 3, 1, 1),
    (2, 8, 8, 512, 512, 3, 1, 1),
    (2, 13, 13, 64, 192, 5, 1, 2),   # AlexNet's 5x5 conv (at 64 input channels)
    (2, 7, 7, 192, 384, 3, 1, 1),    # AlexNet's third conv
]
# AlexNet's shapes on the weight-gradient kernels (the planner's own tile), and its classifier: a 1x1 conv over
# H = W = 1, a few pixels per split, whose wgrad_reduce crops the rows to cout - 28 (the padded last Linear)
WGRAD_ALEXNET = [(2, 13, 13, 64, 192, 5, 1, 2), (2, 7, 7, 192, 384, 3, 1, 1)]
WGRAD_CLASSIFIER = [(5, 1, 1, 128, 128, 1, 1, 0), (130, 1, 1, 192, 256, 1, 1, 0)]
PP_GEOMS = [
    (5, 14, 14, 256, 256, 3, 1, 1),  # 4 tiles of 256 rows, ragged tail, 36 K-steps
    (5, 14, 14, 192, 256, 3, 1, 1),  # 27 K-steps (odd)
    (5, 14, 14, 64, 256, 1, 1, 0),   # one K-step
]
PP_STRIDED_GEOM = (5, 15, 13, 256, 512, 3, 2, 1)  # dgrad: phase 0 two tiles, the others one; compact residual
L1_GEOMS = [(1, 4, 56, 64, 64, 3, 1, 1), (3, 12, 56, 64, 64, 3, 1, 1)]
L1_FALLBACK_GEOM = (2, 9, 56, 64, 64, 3, 1, 1)  # H % 4 != 0: the generic kernel
C64_M = [421, 70005]  # 3 tiles + a 37-row tail; more tiles than resident blocks
C64_FUSED_INT_M = 12544 + 37  # the fused producer-BN form in the exact layer (sum of squares below 2**24)
C64_BNB = [((4, 56, 56), 2, 64), ((4, 56, 56), 3, 64), ((4, 56, 56), 2, 128),
           ((3, 13, 11), 2, 64), ((3, 13, 11), 3, 64), ((3, 13, 11), 2, 128)]  # (N, H, W), mode, cin
X_PLAIN = [(128, 3037), (128, 421)]                      # cin, M (both ragged)
X_STRIDED = [(128, (2, 9, 10)), (256, (3, 13, 11))]      # cin, (N, H, W): odd H / W reads the last row / column
X_BNB = [(128, (2, 28, 28)), (128, (3, 13, 11))]         # cin, (N, H, W): 429 pixels is a ragged tail
GROUPED = [(128, 2, 1, 9), (256, 64, 2, 8)]              # width, groups, stride, H
WGRAD_GENERIC = [(2, 14, 14, 64, 64, 3, 1, 1), (2, 7, 7, 256, 64, 1, 1, 0), (2, 8, 56, 64, 64, 3, 1, 1)]
WGRAD_PAIR = [(3, 6, 6, 64, 128, 3, 2, 1), (2, 9, 9, 64, 384, 1, 1, 0)]
WGRAD_WIDE = [(3, 6, 6, 128, 128, 3, 2, 1), (1, 7, 7, 384, 128, 3, 1, 1)]
WGRAD_PP = [(6, 14, 14, 256, 256, 3, 1, 1)]
WGRAD_L1 = (5, 22, 56)  # conv_wgrad_3x3c64: N, H, W (H % 4 != 0: a partial last row tile)
WGRAD_TARGETS = [64, 2048]
# the 3-channel first conv on the generic window kernels (R, stride, pad, N, H, W): AlexNet's 11x11/4 (two 8-pixel windows
# per kernel row), VGG's 3x3/1, a 5x5/2, and a 9x9/3 (two windows, an odd R: a padding kernel row in the last pair)
FIRST_CONV = [(11, 4, 2, 2, 39, 35), (3, 1, 1, 2, 10, 12), (5, 2, 2, 2, 13, 11), (9, 3, 4, 2, 20, 23)]
STEM = [(3, 32, 32), (65, 32, 32)]  # N, H, W of the image; 65 images: 260 four-row tiles, more than 256 blocks


def c64_geom(M):
    return (1, 1, M, 64, 256, 1, 1, 0)


def x_plain_geom(cin, M):
    return (1, 1, M, cin, 4 * cin, 1, 1, 0)


def x_strided_geom(cin, nhw):
    return (nhw[0], nhw[1], nhw[2], cin, 2 * cin, 1, 2, 0)


def bnb_1x1_geom(nhw, cin, cout):
    """Backward-data of a 1x1 cout -> cin conv: dY has cin channels, dX cout."""
    return (nhw[0], nhw[1], nhw[2], cout, cin, 1, 1, 0)


def grouped_geom(width, groups, stride, H):
    return (2, H, H, width, width, 3, stride, 1)


def out_hw(g):
    N, H, W, C, K, R, st, pad = g
    return (H + 2 * pad - R) // st + 1, (W + 2 * pad - R) // st + 1


def _seed(g, salt):
    return sum((i + 3) * int(v) for i, v in enumerate(g)) * 31 + salt


def _real(shape, gen, dtype, scale=1.0):
    return (torch.randn(*shape, generator=gen) * scale).to(dtype)


def _ints(shape, values, seed, dtype):
    return nm.conv_int_operands(shape, values, seed).to(dtype)


def fwd_operands(g, dtype, layer, narrow=False, residual=False):
    """(x, w, res) of the forward conv; ``narrow``: layer-A activations from {-1, 1} only."""
    N, H, W, C, K, R, st, pad = g
    sd = _seed(g, 1)
    P, Q = out_hw(g)
    if layer == "int":
        x = _ints((N, H, W, C), (-1, 1) if narrow else XVALS, sd, dtype)
        w = _ints((K, R, R, C), WVALS, sd + 1, dtype)
        res = _ints((N, P, Q, K), XVALS, sd + 2, dtype) if residual else None
        return x, w, res
    gen = torch.Generator().manual_seed(sd)
    x = _real((N, H, W, C), gen, dtype)
    wf = torch.randn(K, R, R, C, generator=gen) * (1.0 / (C * R * R)) ** 0.5
    rf = torch.randn(N, P, Q, K, generator=gen) if residual else None
    if dtype in SMALL_CHANNEL:
        wf[1] *= 1e-3
        if residual:
            rf[..., 1] *= 1e-3
    return x, wf.to(dtype), (rf.to(dtype) if residual else None)


def dgrad_operands(g, dtype, layer, residual=None, narrow=False):
    """(dy, w, res) of the backward-data conv; ``residual``: None | "full" ([N, H, W, C]) | "compact" (phase (0, 0):
    [N, ceil(H / stride), ceil(W / stride), C])."""
    N, H, W, C, K, R, st, pad = g
    sd = _seed(g, 11)
    P, Q = out_hw(g)
    rshape = None
    if residual == "full":
        rshape = (N, H, W, C)
    elif residual == "compact":
        rshape = (N, -(-H // st), -(-W // st), C)
    if layer == "int":
        dy = _ints((N, P, Q, K), (-1, 1) if narrow else XVALS, sd, dtype)
        w = _ints((K, R, R, C), WVALS, sd + 1, dtype)
        res = _ints(rshape, XVALS, sd + 2, dtype) if rshape else None
        return dy, w, res
    gen = torch.Generator().manual_seed(sd)
    dy = _real((N, P, Q, K), gen, dtype)
    wf = torch.randn(K, R, R, C, generator=gen) * (1.0 / (K * R * R)) ** 0.5
    rf = torch.randn(*rshape, generator=gen) if rshape else None
    if dtype in SMALL_CHANNEL:
        wf[..., 1] *= 1e-3
        if rf is not None:
            rf[..., 1] *= 1e-3
    return dy, wf.to(dtype), (rf.to(dtype) if rf is not None else None)


def wgrad_operands(g, dtype, layer):
    N, H, W, C, K, R, st, pad = g
    sd = _seed(g, 21)
    P, Q = out_hw(g)
    if layer == "int":
        return _ints((N, H, W, C), XVALS, sd, dtype), _ints((N, P, Q, K), XVALS, sd + 1, dtype)
    gen = torch.Generator().manual_seed(sd)
    return _real((N, H, W, C), gen, dtype), _real((N, P, Q, K), gen, dtype)


def bnb_operands(mode, shape, dtype, layer, seed=0):
    """Operands of the fused BN-backward epilogue of a data gradient of NHWC ``shape``: dict with y1, coef1
    ([scale | shift | mean | invstd], fp32), y2 / coef2 (mode 3: a branch of its own) and ``out`` (modes 2, 3: the block
    output whose sign is the ReLU mask).  Layer A: integer y and mean, power-of-two invstd (0.25 .. 2 over the
    channels), scale +-{1, 2, 4} and shift 0.5 (the pre-activation is an integer plus a half: never zero), so every sum
    is exact."""
    C = shape[-1]
    sd = 1000 * mode + 7 * C + seed
    gen = torch.Generator().manual_seed(sd)
    d = {"y2": None, "coef2": None, "out": None}

    def branch(k):
        if layer == "int":
            y = _ints(shape, XVALS, sd + 10 * k, dtype)
            ch = torch.arange(C)
            scale = torch.tensor([1.0, 2.0, 4.0])[(ch + k) % 3]
            sign = torch.where((ch // 3 + k) % 2 == 0, 1.0, -1.0)
            mean = ((ch + 2 * k) % 3 - 1).float()
            invstd = torch.tensor([0.25, 0.5, 1.0, 2.0])[(ch // 2 + k) % 4]
            return y, torch.cat([scale * sign, torch.full((C,), 0.5), mean, invstd]).contiguous()
        y = _real(shape, gen, dtype)
        yf = y.float().view(-1, C)
        coef = torch.cat([torch.rand(C, generator=gen) + 0.5, torch.randn(C, generator=gen) * 0.3, yf.mean(0),
                          torch.rsqrt(yf.var(0, unbiased=False) + 1e-5)]).contiguous()
        return y, coef
    d["y1"], d["coef1"] = branch(1)
    if mode == 3:
        d["y2"], d["coef2"] = branch(2)
    if mode > 1:
        d["out"] = torch.relu(torch.randn(*shape, generator=gen)).to(dtype)
    return d


def bnb_mask(mode, d, C):
    """fp64-side ReLU mask of the epilogue and, for mode 1, the pre-activation with its magnitude (the elements whose
    sign fp32 cannot be trusted with are those with |pre| <= 8u * mag)."""
    if mode == 1:
        c64 = d["coef1"].to(torch.float64)
        t = d["y1"].to(torch.float64).reshape(-1, C) * c64[:C]
        pre, mag = t + c64[C:2 * C], t.abs() + c64[C:2 * C].abs()
        return pre > 0, pre.abs() <= 8 * nm.U * mag
    m = d["out"].to(torch.float64).reshape(-1, C) > 0
    return m, torch.zeros_like(m)


def pre_operands(layer, dtype, seed=5):
    """[scale | shift | 0 | 0] x 64 of a fused producer BN + ReLU.  Layer A: scale from {1, 2}, integer shift."""
    gen = torch.Generator().manual_seed(seed)
    if layer == "int":
        ch = torch.arange(64)
        scale, shift = (ch % 2 + 1).float(), ((ch // 2) % 3 - 1).float()
    else:
        scale, shift = torch.rand(64, generator=gen) + 0.5, torch.randn(64, generator=gen) * 0.5
    return torch.cat([scale, shift, torch.zeros(128)]).contiguous()


def stem_operands(N, H, W, dtype, layer):
    """(fp32 NCHW image, KRSC 7x7 weight [64, 7, 7, 3] in ``dtype``)."""
    if layer == "int":
        return nm.conv_int_operands((N, 3, H, W), XVALS, 41), nm.conv_int_operands((64, 7, 7, 3), WVALS, 42).to(dtype)
    gen = torch.Generator().manual_seed(43)
    return torch.randn(N, 3, H, W, generator=gen), (torch.randn(64, 7, 7, 3, generator=gen) * 0.05).to(dtype)


def first_conv_geom(case):
    R, st, pad, N, H, W = case
    return (N, H, W, 3, 64, R, st, pad)


def first_conv_operands(case, dtype, layer):
    """(fp32 NCHW image, KRSC weight [64, R, R, 3] in ``dtype``, dY [N, P, Q, 64] in ``dtype``) of a ``FIRST_CONV``
    case."""
    R, st, pad, N, H, W = case
    P, Q = out_hw(first_conv_geom(case))
    sd = 300 + 17 * R + H
    if layer == "int":
        return (nm.conv_int_operands((N, 3, H, W), XVALS, sd), nm.conv_int_operands((64, R, R, 3), WVALS, sd + 1).to(dtype),
                nm.conv_int_operands((N, P, Q, 64), XVALS, sd + 2).to(dtype))
    gen = torch.Generator().manual_seed(sd)
    w = torch.randn(64, R, R, 3, generator=gen) * (1.0 / (3 * R * R)) ** 0.5
    if dtype in SMALL_CHANNEL:
        w[1] *= 1e-3
    return torch.randn(N, 3, H, W, generator=gen), w.to(dtype), torch.randn(N, P, Q, 64, generator=gen).to(dtype)


def pre_apply_ref(z, coef, dtype):
    """relu(z * scale + shift) as the fused kernels form it: one fp32 fma, rounded to the 16-bit type."""
    z64 = z.to(torch.float64)
    c64 = coef.to(torch.float64)
    return torch.relu(z64 * c64[:64] + c64[64:128])


def grouped_weights(width, groups, dtype, layer, seed=3):
    """(grouped KRSC weight [width, 3, 3, cg], dense block-diagonal slice weights [width / 64, 64, 3, 3, 64], the full
    dense [width, 3, 3, width] weight of the references)."""
    cg = width // groups
    if layer == "int":
        wg = _ints((width, 3, 3, cg), WVALS, seed, dtype)
    else:
        wg = _real((width, 3, 3, cg), torch.Generator().manual_seed(seed), dtype, (1.0 / (cg * 9)) ** 0.5)
    nsl = width // 64
    dense = torch.zeros(nsl, 64, 3, 3, 64, dtype=dtype)
    full = torch.zeros(width, 3, 3, width, dtype=dtype)
    for k in range(width):
        g0 = (k // cg) * cg
        full[k, :, :, g0:g0 + cg] = wg[k]
        dense[k // 64, k % 64, :, :, g0 % 64:g0 % 64 + cg] = wg[k]
    return wg, dense, full


# ---- every layer-A case: (name, kind, geometry, options) -- test_numerics_model_cpu checks the representability cap
# and the sum-of-squares condition on each of them; test_conv_numerics_gpu runs them.  ``narrow``: activations from
# {-1, 1} (the wider set breaks the 1 % cap at this reduction length).
NARROW = {(2, 8, 8, 512, 512, 3, 1, 1), (2, 13, 13, 64, 192, 5, 1, 2)}  # the second: its data gradient, 4800 terms


def layer_a_cases():
    out = []
    fwd = [TILE_GEOM] + DEFAULT_GEOMS + PP_GEOMS + L1_GEOMS + [L1_FALLBACK_GEOM] + [c64_geom(M) for M in C64_M] \
        + [x_plain_geom(c, M) for c, M in X_PLAIN] + [x_strided_geom(c, nhw) for c, nhw in X_STRIDED]
    for g in fwd:
        out.append(("fwd", g, {}))
    for g in [TILE_GEOM] + DEFAULT_GEOMS + PP_GEOMS[:1] + L1_GEOMS + [L1_FALLBACK_GEOM]:
        out.append(("dgrad", g, {"residual": "full"}))
    out.append(("dgrad", PP_STRIDED_GEOM, {"residual": "compact"}))
    for nhw, mode, cin in C64_BNB:
        out.append(("dgrad", bnb_1x1_geom(nhw, cin, 256), {"residual": "full"}))
    for cin, nhw in X_BNB:
        out.append(("dgrad", bnb_1x1_geom(nhw, cin, 4 * cin), {"residual": "full"}))
    for g in L1_GEOMS + [c64_geom(421), c64_geom(C64_FUSED_INT_M)]:
        out.append(("fwd_pre", g, {}))
    for width, groups, stride, H in GROUPED:
        out.append(("grouped_fwd", grouped_geom(width, groups, stride, H), {"groups": groups}))
        out.append(("grouped_dgrad", grouped_geom(width, groups, stride, H), {"groups": groups}))
    for N, H, W in STEM:
        out.append(("stem", (N, H, W, 3, 64, 7, 2, 3), {}))
    for case in FIRST_CONV:
        out.append(("first", first_conv_geom(case), {}))
    seen, uniq = set(), []
    for kind, g, opt in out:
        key = (kind, g, tuple(sorted(opt.items())))
        if key not in seen:
            seen.add(key)
            uniq.append((kind, g, opt))
    return uniq


# ======================================================================================= the fp32 path (fp32.hip)
# tests/test_conv32_numerics_gpu.py runs these on the kernels, tests/test_numerics_model_cpu.py proves the layer-A
# conditions and the assertions on them.  Three layers: "int" and "real" as above (dtype float32), and "wide": 1x1
# geometries whose every output is exactly one non-zero product that needs the full 24-bit multiply.
C32_TILE_GEOM = (13, 13, 11, 128, 256, 3, 2, 1)      # M = 546: ragged on 128, 256 and 512 rows; dgrad GEMM-N = 128
C32_TILE_GEOM_256 = (13, 13, 11, 256, 64, 3, 2, 1)   # dgrad GEMM-N = 256: the (256, 256) tile
C32_TILES = [(128, 128), (128, 64), (256, 256), (256, 128), (256, 64), (512, 64)]
C32_FWD_VARIANTS = ["plain", "res", "stats", "stats_res"]
# backward-data epilogues: (name, bnb mode of bnb_operands or 0, residual); mode 2: one branch, stored mask reference;
# mode 3: two branches (always a stored mask); mode 1: one branch, the mask recomputed from y1 (bn_mref = None)
C32_EPILOGUES = [("none", 0, False), ("res", 0, True), ("bn1", 2, False), ("bn1_res", 2, True), ("bn2", 3, False),
                 ("bn2_res", 3, True), ("bn1_nomref", 1, False)]
C32_DEFAULT_GEOMS = [
    (2, 14, 9, 64, 64, 3, 1, 1),
    (2, 15, 13, 64, 128, 3, 2, 1),
    (3, 14, 11, 128, 256, 1, 2, 0),  # dgrad: three phases without taps write zeros plus the residual
    (2, 12, 7, 64, 256, 1, 1, 0),
    (1, 9, 5, 96, 128, 3, 1, 1),     # C % 32 only
    (2, 8, 6, 512, 128, 3, 1, 1),
]
# 3x3/s1/p1 on the halo kernel (bn = 64); the reduction has C channels and the output K, in both directions
C32_HALO_GEOMS = [
    (2, 8, 56, 64, 64, 3, 1, 1),    # W at the 464-row limit; tiles start mid-row and cross the image boundary
    (3, 5, 64, 32, 64, 3, 1, 1),    # the isolated admitted width; one channel chunk
    (30, 3, 3, 96, 128, 3, 1, 1),   # one tile spans 28 images; three chunks; two column tiles
    (5, 10, 10, 64, 64, 3, 1, 1),
    (3, 7, 9, 128, 128, 3, 1, 1),
]
C32_HALO_REFUSED = [(2, 8, 57, 64, 64, 3, 1, 1), (3, 5, 2, 64, 64, 3, 1, 1)]  # the restaging kernel must run
W32_T64 = [(2, 9, 7, 64, 64, 3, 1, 1), (3, 6, 5, 64, 128, 3, 2, 1), (2, 7, 5, 192, 64, 1, 1, 0)]
W32_T128 = [(3, 6, 5, 128, 128, 3, 2, 1), (1, 7, 6, 384, 128, 3, 1, 1)]
W32_HALO = [(2, 5, 62, 64, 64, 3, 1, 1), (3, 9, 28, 64, 128, 3, 1, 1), (2, 6, 5, 128, 64, 3, 1, 1),
            (2, 56, 56, 64, 64, 3, 1, 1)]
# window-mode stem images (N, H, W); the last two carry an odd pooled width (9) / an odd conv width (19) and a
# partial last 32-pixel chunk for the fused weight gradient
STEM32 = [(3, 32, 24), (3, 64, 48)]
STEM32_FUSED = STEM32 + [(3, 40, 36), (2, 42, 38)]
STEM32_TILES = [(128, 64), (256, 64), (512, 64)]
WIDE_VARIANTS = ["a", "b", "c"]
WIDE_FWD = [(2, 9, 7, 32, 64, 1, 1, 0), (2, 9, 7, 64, 128, 1, 1, 0)]  # one and two K-steps; 126 pixels: a ragged tile
WIDE_WGRAD = [((1, 8, 8, 64, 64, 1, 1, 0), 64), ((2, 8, 8, 128, 128, 1, 1, 0), 128)]  # N*P*Q == C; (geometry, tile)


def dgrad_geom32(g):
    """The geometry whose backward-data pass reduces over g's ``C`` channels and writes g's ``K``: the listed channel
    counts name (reduction, output) in both directions, and conv32_dgrad needs its output channels % 64 == 0."""
    N, H, W, C, K, R, st, pad = g
    return (N, H, W, K, C, R, st, pad)


def tile32_default(n, m):
    """The tile ResNetExecutor32._tile32 chooses for a GEMM of n columns and m rows."""
    from pytorch_distributed_template_amd.models.executor32 import ResNetExecutor32
    return ResNetExecutor32._tile32(ResNetExecutor32, n, m)


def dgrad_geoms32_default():
    """C32_DEFAULT_GEOMS for backward data: as listed where the output channels allow a 64-wide tile, else swapped."""
    return [g if g[3] % 64 == 0 else dgrad_geom32(g) for g in C32_DEFAULT_GEOMS]


def wgrad32_plans(g, tile, target=1024):
    """Split plans (splits, pix_per_split) of a weight gradient: one split; the plan ResNetExecutor32._wgrad makes for
    ``target`` blocks; a plan whose last split is partial; for the halo tile one output row per split.  (A split that
    owns no pixel at all is produced by no caller and is left out.)"""
    N, H, W, C, K, R, st, pad = g
    P, Q = out_hw(g)
    plans = []
    if tile == 3:
        rows = N * P
        per_split = 3 * (K // 64) * (C // 64)
        s = max(1, min(target // per_split, rows))
        pps = -(-rows // s)
        part = next(p for p in range(2, rows + 2) if rows % p != 0 or p > rows)
        for pp in (rows, pps, part, 1):
            plans.append((-(-rows // pp), pp))
    else:
        npix = N * P * Q
        per_split = (K // tile) * R * R * (C // tile)
        tgt = target if tile == 64 else target // 2
        s = max(1, min(tgt // max(per_split, 1), (npix + 63) // 64))
        pps = (-(-npix // s) + 63) // 64 * 64
        for pp in ((npix + 63) // 64 * 64, pps, 64):
            plans.append((-(-npix // pp), pp))
    return sorted(set(plans))


def wide_pair(shape_act, shape_w, variant, seed):
    """(activation-side, weight-side) fp32 operands of the ``wide`` layer: (a) 12-bit odd integers on both sides -- the
    product needs 23 or 24 bits --, (b) 24-bit odd integers against +-{1, 2, 4}, (c) the mirror of (b)."""
    if variant == "a":
        return nm.wide_operand(shape_act, 12, seed), nm.wide_operand(shape_w, 12, seed + 1)
    if variant == "b":
        return nm.wide_operand(shape_act, 24, seed), nm.wide_small(shape_w, seed + 1)
    return nm.wide_small(shape_act, seed), nm.wide_operand(shape_w, 24, seed + 1)


def wide_fwd_operands(g, variant):
    """(x, w) of a 1x1 forward (or, as (dy, w), of a 1x1 backward-data with g = dgrad_geom32(...)): the activation of
    pixel p is non-zero only in channel (7 p) % C of its reduction channels."""
    N, H, W, C, K, R, st, pad = g
    assert R == 1 and st == 1 and pad == 0
    a, w = wide_pair((N * H * W, C), (K, 1, 1, C), variant, _seed(g, 51))
    p = torch.arange(N * H * W)
    keep = torch.zeros(N * H * W, C)
    keep[p, (7 * p) % C] = 1.0
    return (a * keep).view(N, H, W, C).contiguous(), w


def wide_dgrad_operands(g, variant):
    """(dy [N, H, W, K], w [K, 1, 1, C]) of a 1x1 backward-data: dY of pixel p is non-zero only in channel (7 p) % K."""
    N, H, W, C, K, R, st, pad = g
    assert R == 1 and st == 1 and pad == 0
    a, w = wide_pair((N * H * W, K), (K, 1, 1, C), variant, _seed(g, 52))
    p = torch.arange(N * H * W)
    keep = torch.zeros(N * H * W, K)
    keep[p, (7 * p) % K] = 1.0
    return (a * keep).view(N, H, W, K).contiguous(), w


def wide_wgrad_operands(g, variant):
    """(x, dy) of a 1x1 weight gradient over N*P*Q == C pixels: pixel p carries input channel (7 p) % C alone (7 and C
    are coprime: every channel has exactly one pixel), so dW[k][c] is one product."""
    N, H, W, C, K, R, st, pad = g
    assert R == 1 and st == 1 and pad == 0 and N * H * W == C
    x, dy = wide_pair((C, C), (C, K), variant, _seed(g, 53))
    p = torch.arange(C)
    keep = torch.zeros(C, C)
    keep[p, (7 * p) % C] = 1.0
    return (x * keep).view(N, H, W, C).contiguous(), dy.view(N, H, W, K).contiguous()


def stem32_operands(N, H, W, layer):
    """(fp32 NCHW image, KRSC 7x7 weight [64, 7, 7, 3], dY [N, P, Q, 64]) of the fp32 window-mode stem."""
    P, Q = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    sd = 61 + H * W
    if layer == "int":
        return (nm.conv_int_operands((N, 3, H, W), XVALS, sd), nm.conv_int_operands((64, 7, 7, 3), WVALS, sd + 1),
                nm.conv_int_operands((N, P, Q, 64), XVALS, sd + 2))
    gen = torch.Generator().manual_seed(sd)
    w = torch.randn(64, 7, 7, 3, generator=gen) / 147 ** 0.5
    w[1] *= 1e-3
    return torch.randn(N, 3, H, W, generator=gen), w, torch.randn(N, P, Q, 64, generator=gen)


def stem32_tail_operands(N, P, Q, layer, C=64, seed=0):
    """Operands of the stem's backward tail over the conv output [N, P, Q, C]: dict with y (conv output), dp (pooled
    gradient [N, OH, OW, C]), idx (random argmax codes 0..8, codes that point outside the image included), coef
    ([scale | shift | mean | invstd]) and b ([A | B | Cc]).  Layer A: integer y and dp, scale +-{1, 2, 4}, shift 0.5 (the
    pre-activation is never zero), power-of-two A and B, integer Cc: dY = A*dz + B*y + Cc is exact."""
    OH, OW = (P - 1) // 2 + 1, (Q - 1) // 2 + 1
    gen = torch.Generator().manual_seed(71 + 13 * P + Q + C + seed)
    idx = torch.randint(0, 9, (N, OH, OW, C), generator=gen, dtype=torch.uint8)
    ch = torch.arange(C)
    if layer == "int":
        y = nm.conv_int_operands((N, P, Q, C), XVALS, 72 + P + seed)
        dp = nm.conv_int_operands((N, OH, OW, C), XVALS, 73 + P + seed)
        scale = torch.tensor([1.0, 2.0, 4.0])[ch % 3] * torch.where((ch // 3) % 2 == 0, 1.0, -1.0)
        coef = torch.cat([scale, torch.full((C,), 0.5), ((ch % 3) - 1).float(),
                          torch.tensor([0.25, 0.5, 1.0, 2.0])[(ch // 2) % 4]])
        b = torch.cat([torch.tensor([1.0, 2.0, 0.5])[ch % 3] * torch.where((ch // 2) % 2 == 0, 1.0, -1.0),
                       torch.tensor([2.0, -1.0, 1.0, -2.0])[ch % 4], ((ch % 5) - 2).float()])
    else:
        y = torch.randn(N, P, Q, C, generator=gen)
        dp = torch.randn(N, OH, OW, C, generator=gen)
        sign = torch.where(torch.rand(C, generator=gen) < 0.3, -1.0, 1.0)
        coef = torch.cat([(torch.rand(C, generator=gen) + 0.5) * sign, torch.randn(C, generator=gen) * 0.3,
                          torch.randn(C, generator=gen) * 0.3, torch.rand(C, generator=gen) + 0.5])
        b = torch.cat([(torch.rand(C, generator=gen) + 0.5) * sign.roll(1), torch.randn(C, generator=gen) * 0.2,
                       torch.randn(C, generator=gen) * 0.1])
    return dict(y=y, dp=dp, idx=idx, coef=coef.contiguous(), b=b.contiguous())


def pool_out_hw(P, Q, pad=1):
    """Output size of MaxPool(3, 2, pad) over a P x Q map."""
    return (P + 2 * pad - 3) // 2 + 1, (Q + 2 * pad - 3) // 2 + 1


def stem_tail_operands(N, P, Q, layer, dtype, C=64, seed=0, pad=1):
    """``stem32_tail_operands`` for the 16-bit kernels and MaxPool(3, 2, ``pad``): y and dp are rounded to ``dtype`` (the
    values the kernels read, held as ``dtype`` tensors), and about a tenth of the argmax bytes carry the dead code 255
    (a window whose maximum is the ReLU's zero) next to the codes 0..8, which at pad 1 include positions outside the
    image.  Layer B scales channel 1 of dp, of the scale and of the shift by 1e-3: a small channel cannot hide in a
    norm.  The fp32 operands of ``stem32_tail_operands`` are untouched by this function."""
    OH, OW = pool_out_hw(P, Q, pad)
    d = stem32_tail_operands(N, P, Q, layer, C=C, seed=seed + 1000 * pad + (7 if dtype == torch.float16 else 0))
    gen = torch.Generator().manual_seed(79 + 13 * P + Q + C + seed + 1000 * pad)
    idx = torch.randint(0, 9, (N, OH, OW, C), generator=gen, dtype=torch.uint8)
    idx[torch.rand(N, OH, OW, C, generator=gen) < 0.1] = 255
    if layer == "int":
        dp = nm.conv_int_operands((N, OH, OW, C), XVALS, 74 + P + seed + pad)
    else:
        dp = torch.randn(N, OH, OW, C, generator=gen)
        dp[..., 1] *= 1e-3
        d["coef"][1] *= 1e-3
        d["coef"][C + 1] *= 1e-3
    return dict(y=d["y"].to(dtype), dp=dp.to(dtype), idx=idx, coef=d["coef"].contiguous(), b=d["b"])


# ResNet stem weight gradient in window mode, (T, U) = (4, 1): images (N, H, W).  Plain kernel: an odd conv height and
# width / even ones / a multiple of 4 x 16; fused raw-row kernel: conv output a multiple of 4 x 16; fused quad kernel:
# an odd conv height (half-dead last quads), a pooled width whose last window column is missing, both
STEM_WGRAD_PLAIN = [(2, 29, 28), (3, 28, 36), (5, 32, 32)]
STEM_WGRAD_ROWS = [(2, 8, 32), (5, 32, 32)]
STEM_WGRAD_QUAD = [(2, 29, 28), (3, 28, 36), (5, 29, 36)]


def stem_fused_operands(N, H, W, dtype, layer):
    """Operands of the fused stem weight gradient: dict x (fp32 NCHW image), y (stand-in conv output [N, P, Q, 64]), dp,
    coef, b as ``stem_tail_operands`` makes them, and idx CONSISTENT with y, as bn_relu_maxpool writes it (the fused
    kernels take the ReLU mask from it): the first fp64 argmax of each window, 255 where the maximum is 0; on top a
    tenth of the windows are marked dead and a tenth of the top-row windows carry a code of the row above the image --
    neither routes a gradient, in the kernels or in ``stem_tail_ref``."""
    import _pool_cases as pc
    P, Q = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    d = stem_tail_operands(N, P, Q, layer, dtype, C=64, seed=H + W)
    r = pc.pool_fwd_ref(d["y"], d["coef"], 3, 1)
    idx = torch.where(r["ref"] > 0, r["first"], torch.full_like(r["first"], 255)).to(torch.uint8)
    gen = torch.Generator().manual_seed(83 + H * W)
    idx[torch.rand(idx.shape, generator=gen) < 0.1] = 255
    top = torch.rand(idx[:, 0].shape, generator=gen) < 0.1
    idx[:, 0] = torch.where(top, torch.randint(0, 3, idx[:, 0].shape, generator=gen, dtype=torch.uint8), idx[:, 0])
    x = nm.conv_int_operands((N, 3, H, W), XVALS, 84 + H) if layer == "int" else torch.randn(N, 3, H, W, generator=gen)
    return dict(d, idx=idx, x=x)


def stem_tail_ref(d, N, P, Q, C, pad=1):
    """Independent fp64 reference of the stem's backward tail from ``stem32_tail_operands`` / ``stem_tail_operands``
    (any device; MaxPool(3, 2, ``pad``)): the pooled gradient scattered along the argmax bytes (the dead code 255 and
    codes pointing outside the image select nothing), the ReLU mask from
    y*scale + shift, dY = A*dz + B*y + Cc.  Returns dict dz, dzmag (scatter of |dp|), unsure (|pre| <= 8u*mag: the sign
    fp32 may call either way), dy, dymag (|A|*dzmag + |B*y| + |Cc|), dyflip (|A|*dzmag where unsure, else 0)."""
    y, dp, idx = d["y"], d["dp"], d["idx"]
    dev = y.device
    OH, OW = pool_out_hw(P, Q, pad)
    dz = torch.zeros(N, P, Q, C, dtype=torch.float64, device=dev)
    dzmag = torch.zeros_like(dz)
    n_i, oh_i, ow_i, c_i = torch.meshgrid(*[torch.arange(s, device=dev) for s in (N, OH, OW, C)], indexing="ij")
    h = oh_i * 2 - pad + (idx // 3).long()
    w = ow_i * 2 - pad + (idx % 3).long()
    ok = (idx < 9) & (h >= 0) & (h < P) & (w >= 0) & (w < Q)
    flat = ((n_i * P + h) * Q + w) * C + c_i
    dz.view(-1).index_put_((flat[ok],), dp.double()[ok], accumulate=True)
    dzmag.view(-1).index_put_((flat[ok],), dp.double().abs()[ok], accumulate=True)
    c64 = d["coef"].double()
    t1, t2 = y.double() * c64[:C], c64[C:2 * C]
    pre = t1 + t2
    unsure = pre.abs() <= 8 * nm.U * (t1.abs() + t2.abs())
    dzraw = dz
    dz = torch.where(pre > 0, dz, torch.zeros_like(dz))
    b64 = d["b"].double()
    A, B, Cc = b64[:C], b64[C:2 * C], b64[2 * C:3 * C]
    dy = A * dz + B * y.double() + Cc
    dymag = A.abs() * dzmag + (B * y.double()).abs() + Cc.abs()
    dyflip = torch.where(unsure, A.abs() * dzmag, torch.zeros_like(dzmag))
    return dict(dz=dz, dzraw=dzraw, dzmag=dzmag, unsure=unsure, dy=dy, dymag=dymag, dyflip=dyflip)


def layer_a_cases32():
    """Every fp32 layer-A case: (kind, geometry, options)."""
    out = [("fwd", C32_TILE_GEOM, {"residual": True})]
    out += [("dgrad", g, {"residual": "full"}) for g in (C32_TILE_GEOM, C32_TILE_GEOM_256)]
    out += [("fwd", g, {"residual": True}) for g in C32_DEFAULT_GEOMS + C32_HALO_GEOMS + C32_HALO_REFUSED]
    out += [("dgrad", g, {"residual": "full"}) for g in dgrad_geoms32_default()]
    out += [("dgrad", dgrad_geom32(g), {"residual": "full"}) for g in C32_HALO_GEOMS + C32_HALO_REFUSED]
    out += [("wgrad", g, {}) for g in W32_T64 + W32_T128 + W32_HALO]
    out += [("stem", (N, H, W, 3, 64, 7, 2, 3), {}) for N, H, W in STEM32_FUSED]
    return out
