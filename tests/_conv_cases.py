"""The conv cases and operands shared by tests/test_conv_numerics_gpu.py (the kernels) and
tests/test_numerics_model_cpu.py (the error model): one list, so the two cannot drift apart (a plain module).

A geometry is ``(N, H, W, C, K, R, stride, pad)``: NHWC input [N, H, W, C], KRSC weight [K, R, R, C].  Operands are
made on the CPU generator and are the same numbers wherever they are used.

Layer A (``layer="int"``): activations, gradients and residuals from {-2, -1, 1, 2}, weights from {-1, 1}: no zeros,
so every dropped, doubled or misplaced term changes the integer result, and every partial sum is exact in fp32.
Layer B (``layer="real"``): randn rounded to the dtype, weights scaled by (reduction length)**-0.5; fp16 cases scale
one output channel by 1e-3 so its outputs approach the subnormal range.
"""
import torch

import _numerics as nm

DTYPES = [torch.bfloat16, torch.float16]
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
]
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
    if dtype == torch.float16:
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
    if dtype == torch.float16:
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
NARROW = {(2, 8, 8, 512, 512, 3, 1, 1)}


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
    seen, uniq = set(), []
    for kind, g, opt in out:
        key = (kind, g, tuple(sorted(opt.items())))
        if key not in seen:
            seen.add(key)
            uniq.append((kind, g, opt))
    return uniq
