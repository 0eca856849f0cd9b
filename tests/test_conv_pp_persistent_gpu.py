"""Persistent ping-pong conv (conv_pp_kernel): the tile walk must not change a single bit.

Every case runs with the workgroup cap (``max_wg``) at 1, 2 and 3 -- one workgroup walks every tile; uneven shares;
every tile boundary crossed with a prefetched K-step 0 -- and at a cap above the item count, which is the
one-tile-per-workgroup schedule with no prefetch.  Outputs and statistics sums must be ``torch.equal`` across caps;
the uncapped run is also held to the fp32 reference at the bounds of ``test_conv_pp_long_k_and_fused_bn_backward``
(``_rel < 1e-2``; statistics ``rtol=1e-3, atol=1e-2``).  Shapes are the smallest at which each hazard shows: several
tiles with a ragged tail, even / odd / single K-step counts (the prefetch buffer follows the K-step parity), the
512 x 128 tile (no spare LDS), phases with unequal tile counts (slots that only zero a statistics row) and phases
without taps (tiles with no K loop at all).
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
CAPS = [1, 2, 3, 4096]  # 4096 > every case's item count: one tile per workgroup
PP_TILES = [(256, 256, 64), (512, 128, 64)]
DTYPES = [torch.bfloat16, torch.float16]


def _rel(a, b):
    a, b = a.float(), b.float()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-6)).item()


def _rand16(*shape, dtype=torch.bfloat16, scale=1.0):
    return (torch.randn(*shape, device=DEV) * scale).to(dtype)


def _same_across_caps(run):
    """run(cap) -> tuple of tensors; returns the uncapped result after asserting every cap gives the same bits."""
    base = run(CAPS[-1])
    for cap in CAPS[:-1]:
        got = run(cap)
        for i, (g, b) in enumerate(zip(got, base)):
            assert torch.equal(g, b), f"max_wg={cap}: result {i} differs from the one-tile-per-workgroup schedule"
    return base


# N, H, W, C, K, R, pad, tile
FWD_CASES = [
    (5, 14, 14, 256, 256, 3, 1, (256, 256, 64)),  # M = 980: 4 tiles, ragged tail; 36 K-steps (even)
    (5, 14, 14, 192, 256, 3, 1, (256, 256, 64)),  # 27 K-steps (odd: the prefetch buffer alternates per tile)
    (5, 14, 14, 64, 256, 1, 0, (256, 256, 64)),   # one K-step: prefetch, only K-step and scratch meet
    (6, 14, 14, 256, 128, 3, 1, (512, 128, 64)),  # M = 1176: 3 tiles, ragged tail, all 160 KB of LDS in use
    (6, 14, 14, 64, 128, 1, 0, (512, 128, 64)),   # ... with one K-step
]


@pytest.mark.parametrize("case", FWD_CASES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_pp_persistent_forward_stats(case, dtype):
    from pytorch_distributed_template_amd.ops import conv
    N, H, W, C, K, R, pad, tile = case
    torch.manual_seed(3)
    x = _rand16(N, H, W, C, dtype=dtype)
    w = _rand16(K, R, R, C, dtype=dtype, scale=(1.0 / (C * R * R)) ** 0.5)

    def run(cap):
        y, (s, ss) = conv.conv_fwd(x, w, 1, pad, stats=True, tile=tile, max_wg=cap)
        return y, s, ss

    y, s, ss = _same_across_caps(run)
    ref = F.conv2d(x.float().permute(0, 3, 1, 2), w.float().permute(0, 3, 1, 2), padding=pad).permute(0, 2, 3, 1)
    assert _rel(y, ref) < 1e-2
    yf = y.float().reshape(-1, K)
    assert torch.allclose(s.float(), yf.sum(0), rtol=1e-3, atol=1e-2)
    assert torch.allclose(ss.float(), (yf * yf).sum(0), rtol=1e-3, atol=1e-2)


def _bn_operands(mode, N, H, W, C, dtype):
    """The fused BN-backward epilogue's operands, as test_conv_pp_long_k_and_fused_bn_backward builds them."""
    y1 = _rand16(N, H, W, C, dtype=dtype)
    yf1 = y1.float().view(-1, C)
    m1, i1 = yf1.mean(0), torch.rsqrt(yf1.var(0, unbiased=False) + 1e-5)
    coef1 = torch.cat([torch.rand(C, device=DEV) + 0.5, torch.randn(C, device=DEV) * 0.3, m1, i1]).contiguous()
    y2 = _rand16(N, H, W, C, dtype=dtype) if mode == 3 else None
    out = torch.relu(_rand16(N, H, W, C, dtype=dtype)) if mode > 1 else None
    return y1, m1, i1, coef1, y2, out


def _check_bn_sums(mode, sums, dz, y1, y2, m1, i1, C):
    dzf = dz.float().view(-1, C).double()
    x1 = ((y1.float() - m1) * i1).view(-1, C).double()
    assert torch.allclose(sums[:, 0], dzf.sum(0), rtol=1e-3, atol=1e-2)
    assert torch.allclose(sums[:, 1], (dzf * x1).sum(0), rtol=1e-3, atol=1e-2)
    if mode == 3:
        x2 = ((y2.float() - m1) * i1).view(-1, C).double()
        assert torch.allclose(sums[:, 3], (dzf * x2).sum(0), rtol=1e-3, atol=1e-2)


@pytest.mark.parametrize("tile", PP_TILES)
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("dtype", DTYPES)
def test_pp_persistent_dgrad_fused_epilogues(tile, mode, dtype):
    """Stride-1 backward-data, 3x3 256 -> 256 at N = 5 (M = 980), every fused epilogue (mode 0: plain + residual)."""
    from pytorch_distributed_template_amd.ops import conv, native
    N, H, W, C, K = 5, 14, 14, 256, 256
    torch.manual_seed(21 + mode)
    w = _rand16(K, 3, 3, C, dtype=dtype, scale=(1.0 / (C * 9)) ** 0.5)
    dy = _rand16(N, H, W, K, dtype=dtype)
    res = _rand16(N, H, W, C, dtype=dtype) if mode != 1 else None
    plain = torch.nn.grad.conv2d_input((N, C, H, W), w.float().permute(0, 3, 1, 2), dy.float().permute(0, 3, 1, 2),
                                       padding=1).permute(0, 2, 3, 1)
    if res is not None:
        plain = plain + res.float()
    if mode == 0:
        (dx,) = _same_across_caps(lambda cap: (conv.conv_dgrad(dy, w, H, W, 1, 1, residual=res, tile=tile, max_wg=cap),))
        assert _rel(dx, plain) < 1e-2
        return
    y1, m1, i1, coef1, y2, out = _bn_operands(mode, N, H, W, C, dtype)
    coef2 = coef1 if mode == 3 else None
    om = conv.pack_relu_mask(out) if mode > 1 else None
    K_ = 4 if mode == 3 else 2

    def run(cap):
        slots = torch.zeros(native.C.stat_slots() * C * K_, dtype=torch.float64, device=DEV)
        dz = conv.conv_dgrad(dy, w, H, W, 1, 1, residual=res, bnb=(mode, y1, coef1, y2, coef2, om, slots), tile=tile,
                             max_wg=cap)
        return dz, slots.view(-1, C, K_).sum(0)

    dz, sums = _same_across_caps(run)
    mask = ((y1.float() * coef1[:C] + coef1[C:2 * C]) > 0) if mode == 1 else (out.float() > 0)
    assert _rel(dz, plain * mask) < 1e-2
    _check_bn_sums(mode, sums, dz, y1, y2, m1, i1, C)


# N = 4: every phase of the 15 x 13 image is one 256-pixel tile (224, 192, 196 and 168 GEMM rows); N = 5: phase 0 has
# 280 rows -> two tiles and the others one, so three grid slots only zero their statistics row
@pytest.mark.parametrize("N", [4, 5])
@pytest.mark.parametrize("variant", ["plain", "compact_res", "compact_res_bn"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_pp_persistent_dgrad_strided_phases(N, variant, dtype):
    """3x3/2 backward-data, 15 x 13, 256 -> 512: plain, with a compact residual on res_phase=0, and with that plus
    the block-output BN-backward epilogue (per-(phase, tile) statistics rows, some of them only zeroed)."""
    from pytorch_distributed_template_amd.ops import conv, native
    H, W, C, K = 15, 13, 256, 512
    tile = (256, 256, 64)
    torch.manual_seed(12)
    P, Q = conv.out_hw(H, W, 3, 3, 2, 1)
    dy = _rand16(N, P, Q, K, dtype=dtype)
    w = _rand16(K, 3, 3, C, dtype=dtype, scale=(1.0 / (K * 9)) ** 0.5)
    ref = torch.nn.grad.conv2d_input((N, C, H, W), w.float().permute(0, 3, 1, 2), dy.float().permute(0, 3, 1, 2),
                                     stride=2, padding=1).permute(0, 2, 3, 1)
    if variant == "plain":
        (dx,) = _same_across_caps(lambda cap: (conv.conv_dgrad(dy, w, H, W, 2, 1, tile=tile, max_wg=cap),))
        assert _rel(dx, ref) < 1e-2
        return
    dyd = _rand16(N, P, Q, K, dtype=dtype)
    wd = _rand16(K, 1, 1, C, dtype=dtype, scale=(1.0 / K) ** 0.5)
    rc = conv.conv_dgrad(dyd, wd, P, Q, 1, 0)  # the downsample's data gradient on the compact P x Q grid
    ref = ref + torch.nn.grad.conv2d_input((N, C, H, W), wd.float().permute(0, 3, 1, 2),
                                           dyd.float().permute(0, 3, 1, 2), stride=2, padding=0).permute(0, 2, 3, 1)
    # (the reference adds the fp32 downsample gradient; rc is its 16-bit rounding, inside the 1e-2 bound as in
    # test_conv_dgrad_compact_phase_residual)
    if variant == "compact_res":
        (dx,) = _same_across_caps(
            lambda cap: (conv.conv_dgrad(dy, w, H, W, 2, 1, residual=rc, res_phase=0, tile=tile, max_wg=cap),))
        assert _rel(dx, ref) < 1e-2
        return
    mode = 2
    y1, m1, i1, coef1, _, out = _bn_operands(mode, N, H, W, C, dtype)
    om = conv.pack_relu_mask(out)

    def run(cap):
        slots = torch.zeros(native.C.stat_slots() * C * 2, dtype=torch.float64, device=DEV)
        dz = conv.conv_dgrad(dy, w, H, W, 2, 1, residual=rc, res_phase=0, tile=tile, max_wg=cap,
                             bnb=(mode, y1, coef1, None, None, om, slots))
        return dz, slots.view(-1, C, 2).sum(0)

    dz, sums = _same_across_caps(run)
    assert _rel(dz, ref * (out.float() > 0)) < 1e-2
    _check_bn_sums(mode, sums, dz, y1, None, m1, i1, C)


@pytest.mark.parametrize("dtype", DTYPES)
def test_pp_persistent_dgrad_1x1_stride2_empty_phases(dtype):
    """Backward-data of a 1x1/2 conv (512 -> 256, N = 5, 14 x 14): three of the four phases have no taps, so their
    tiles run no K loop and write zeros."""
    from pytorch_distributed_template_amd.ops import conv
    N, H, W, C, K = 5, 14, 14, 256, 512
    tile = (256, 256, 64)
    torch.manual_seed(7)
    dy = _rand16(N, 7, 7, K, dtype=dtype)
    w = _rand16(K, 1, 1, C, dtype=dtype, scale=(1.0 / K) ** 0.5)
    (dx,) = _same_across_caps(lambda cap: (conv.conv_dgrad(dy, w, H, W, 2, 0, tile=tile, max_wg=cap),))
    ref = torch.nn.grad.conv2d_input((N, C, H, W), w.float().permute(0, 3, 1, 2), dy.float().permute(0, 3, 1, 2),
                                     stride=2, padding=0).permute(0, 2, 3, 1)
    assert _rel(dx, ref) < 1e-2
    assert dx[:, 1::2].abs().max().item() == 0 and dx[:, :, 1::2].abs().max().item() == 0
