"""The shared channel-column reducer (csrc/kernels/col_reduce.h) at the widths and row counts its users' own tests do
not reach: the pooled BN-backward reduces beyond C = 64, and row blocks that own no row.

A 256-thread block is C / G channel groups (G = 8 for 16-bit, 4 for fp32) by rpi = 256 // (C / G) row lanes; a thread's
fp32 chain is ceil(rows / (blocks * rpi)) additions long and the block then sums its rpi lanes in fp32, so
``n_chain = ceil(rows / (blocks * rpi)) + rpi`` (tests/_numerics.py).  The cases reach 256 row lanes, 85 lanes with one
idle thread, 10 lanes with 16 idle threads, one lane per block, and fewer rows than lanes.

References are the kernels' own formulas in fp64 from the fp32 coefficients and the very values the kernel reads:
``dz = dp * [out > 0]``, ``a = (out - shift) / scale``, ``xhat = (a - mean) * invstd``.  sum dz is bounded by
``nm.assert_sum``; sum dz * xhat by ``(n_chain + 8) * u * mag`` with ``mag = sum |dz| * invstd * (|a| + |mean|)``: a
term passes through at most seven fp32 roundings (the reciprocal of scale, the difference out - shift, two products, the
subtraction of the mean against the uncancelled magnitude |a| + |mean|, the product with invstd and the product with
dz) and one is added as margin; a plain fp32 evaluation on the CPU at these widths stayed within 4.7 * u * mag per term
in bf16, fp16 and fp32.
"""
import math

import pytest
import torch

import _numerics as nm
from _numerics import U

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]


def _C():
    from pytorch_distributed_template_amd.ops import native
    return native.C


def _nan_slots(C, K):
    return torch.full((_C().stat_slots() * C * K,), float("nan"), dtype=torch.float64, device=DEV)


def _coef4(C):
    """[scale | shift | mean | invstd], all different per channel (tests/test_bn_chain_gpu.py's, tiny=False)."""
    sign = torch.where(torch.rand(C, device=DEV) < 0.3, -1.0, 1.0)
    return torch.cat([(torch.rand(C, device=DEV) + 0.5) * sign, torch.randn(C, device=DEV) * 0.3,
                      torch.randn(C, device=DEV) * 0.3, torch.rand(C, device=DEV) + 0.5]).contiguous()


def _n_chain(rows, blocks, rpi):
    return math.ceil(rows / (blocks * rpi)) + rpi


def _check_slots(slots, C, K, blocks, name):
    """Every entry written (the slots start as NaN); a slot that owns no block partial is zero.  Returns [C, K]."""
    S = _C().stat_slots()
    assert bool(torch.isfinite(slots).all()), f"{name}: slot entries left unwritten"
    sl3 = slots.view(S, C, K)
    for s in range(S):  # slot s owns the block partials [s*blocks/S, (s+1)*blocks/S)
        if s * blocks // S == (s + 1) * blocks // S:
            assert not bool(sl3[s].any()), f"{name}: slot {s} owns no block but is not zero"
    return sl3.sum(0)


# ------------------------------------------------------------------------------------- the pooled reduces
def _pooled_case(rows, C, dtype):
    """out = relu(y * scale + shift) rounded to dtype, dp random; the fp64 reference sums and their bounds' mags."""
    coef = _coef4(C)
    y = torch.randn(rows, C, device=DEV)
    out = torch.relu(y * coef[:C] + coef[C:2 * C]).to(dtype)
    dp = torch.randn(rows, C, device=DEV).to(dtype)
    c64 = coef.double()
    scale, shift, mean, invstd = c64[:C], c64[C:2 * C], c64[2 * C:3 * C], c64[3 * C:]
    o64 = out.double()
    dz = dp.double() * (o64 > 0)
    a = (o64 - shift) / scale
    ref = torch.stack([dz.sum(0), (dz * ((a - mean) * invstd)).sum(0)], 1)
    mag = torch.stack([dz.abs().sum(0), (dz.abs() * invstd * (a.abs() + mean.abs())).sum(0)], 1)
    return dp, out, coef, ref, mag


def _assert_pooled(got, ref, mag, n_chain, name):
    nm.assert_sum(got[:, 0], ref[:, 0], mag[:, 0], n_chain, f"{name}: sum dz", family="col_reduce")
    nm.assert_within(got[:, 1], ref[:, 1], (n_chain + 8) * U * mag[:, 1], f"{name}: sum dz*xhat", family="col_reduce")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,C", [(1, 8), (300, 8), (300, 24), (41, 192), (300, 512), (5, 2048)])
def test_pooled_bwd_reduce_width_and_row_edges(rows, C, dtype):
    torch.manual_seed(rows * 7 + C)
    dp, out, coef, ref, mag = _pooled_case(rows, C, dtype)
    rpi = 256 // (C // 8)
    blocks = min(2048, -(-rows // (rpi * 8)))  # >= 8 rows per thread, at most 2048 blocks
    slots = _nan_slots(C, 2)
    _C().pooled_bwd_reduce(dp, out, coef, slots, rows, C)
    name = f"pooled_bwd_reduce ({rows}, {C}) {dtype}"
    _assert_pooled(_check_slots(slots, C, 2, blocks, name), ref, mag, _n_chain(rows, blocks, rpi), name)


def _run_out32(dp, out, coef, blocks, C, name):
    slots = _nan_slots(C, 2)
    _C().stem_pool_bwd_reduce_out32(dp, out, coef, slots, blocks, C)
    return _check_slots(slots, C, 2, blocks, name)


@pytest.mark.parametrize("rows,C,blocks", [(1, 4, 1), (300, 4, 5), (77, 64, 1), (37, 1024, 5)])
def test_stem_pool_bwd_reduce_out32_width_and_row_edges(rows, C, blocks):
    torch.manual_seed(rows * 7 + C)
    dp, out, coef, ref, mag = _pooled_case(rows, C, torch.float32)
    name = f"stem_pool_bwd_reduce_out32 ({rows}, {C}, {blocks})"
    _assert_pooled(_run_out32(dp, out, coef, blocks, C, name), ref, mag, _n_chain(rows, blocks, 256 // (C // 4)), name)


# ------------------------------------------------------------------------------------- the plan behind bnact
# C -> (row lanes, column chunks) of bnact's plan: the chunk width that idles the fewest lanes (ties: the wider)
BNACT_LANES = {8: (256, 1), 24: (85, 1), 64: (32, 1), 192: (32, 3), 1280: (8, 5), 2048: (1, 1)}


@pytest.mark.parametrize("rows,C", [(1, 8), (5000, 8), (5000, 24), (5000, 64), (5000, 192), (5000, 1280), (60000, 1280),
                                    (5000, 2048)])
def test_bnact_stats_block_counts(rows, C):
    """>= 16 rows per thread, at most 2048 // chunks row blocks ((60000, 1280) is capped at 409): the counts are part
    of the result bits, so an edit of the shared plan must not move them."""
    lanes, chunks = BNACT_LANES[C]
    x = torch.zeros(rows, C, device=DEV, dtype=torch.bfloat16)
    got = _C().bnact_stats(x, _nan_slots(C, 2), rows, C)
    assert list(got) == [max(1, min(2048 // chunks, -(-rows // (lanes * 16)))), lanes]


# ------------------------------------------------------------------------------------- blocks that own no row
def _bn_case(rows, C, dtype):
    """g, y1, y2, a ReLU reference / its bitmask, two coefficient sets and the fp64 [C, 4] sums of bn_bwd_reduce."""
    g = torch.randn(rows, C, device=DEV).to(dtype)
    ys = [(torch.randn(rows, C, device=DEV) * s).to(dtype) for s in (1.5, 0.7)]
    coefs = [_coef4(C), _coef4(C)]
    keep = torch.rand(rows, C, device=DEV) < 0.6
    dz = g.double() * keep
    ref, mag = [], []
    for y, coef in zip(ys, coefs):
        c64 = coef.double()
        t = dz * ((y.double() - c64[2 * C:3 * C]) * c64[3 * C:])
        ref += [dz.sum(0), t.sum(0)]
        mag += [dz.abs().sum(0), t.abs().sum(0)]
    return g, ys, coefs, keep, torch.stack(ref, 1), torch.stack(mag, 1)


def _assert_empty_blocks(run, ref, mag, rows, rpi, name):
    """``run(blocks)`` -> [C, K] slot totals: 7 blocks over 3 rows (blocks 1..6 own no row and must still write a zero
    partial row) within the chain bound of the reference and of the one-block total."""
    one, seven = run(1), run(7)
    n_chain = max(_n_chain(rows, 1, rpi), _n_chain(rows, 7, rpi))
    nm.assert_sum(one, ref, mag, n_chain, f"{name} blocks=1", family="col_reduce")
    nm.assert_sum(seven, ref, mag, n_chain, f"{name} blocks=7", family="col_reduce")
    nm.assert_sum(seven, one, mag, n_chain, f"{name} blocks=7 against blocks=1", family="col_reduce")


@pytest.mark.parametrize("dtype", DTYPES)
def test_bn_bwd_reduce_blocks_without_rows(dtype):
    rows, C = 3, 128
    torch.manual_seed(11)
    g, ys, coefs, keep, ref, mag = _bn_case(rows, C, dtype)
    bit = (1 << torch.arange(8, device=DEV)).to(torch.int32)
    mask = (keep.view(-1, 8).to(torch.int32) * bit).sum(1).to(torch.uint8)

    def run(blocks):
        slots = _nan_slots(C, 4)
        _C().bn_bwd_reduce(g, mask, ys[0], coefs[0], ys[1], coefs[1], slots, blocks, rows, C)
        return _check_slots(slots, C, 4, blocks, f"bn_bwd_reduce blocks={blocks}")

    _assert_empty_blocks(run, ref, mag, rows, 256 // (C // 8), f"bn_bwd_reduce {dtype}")


def test_bn_bwd_reduce32_blocks_without_rows():
    rows, C = 3, 64
    torch.manual_seed(12)
    g, ys, coefs, keep, ref, mag = _bn_case(rows, C, torch.float32)
    mref = keep.float()  # the post-ReLU reference: dz = g where it is > 0

    def run(blocks):
        slots = _nan_slots(C, 4)
        _C().bn_bwd_reduce32(g, mref, ys[0], coefs[0], ys[1], coefs[1], slots, blocks, rows, C)
        return _check_slots(slots, C, 4, blocks, f"bn_bwd_reduce32 blocks={blocks}")

    _assert_empty_blocks(run, ref, mag, rows, 256 // (C // 4), "bn_bwd_reduce32")


def test_stem_pool_bwd_reduce_out32_blocks_without_rows():
    rows, C = 3, 64
    torch.manual_seed(13)
    dp, out, coef, ref, mag = _pooled_case(rows, C, torch.float32)
    rpi = 256 // (C // 4)
    one = _run_out32(dp, out, coef, 1, C, "stem_pool_bwd_reduce_out32 blocks=1")
    seven = _run_out32(dp, out, coef, 7, C, "stem_pool_bwd_reduce_out32 blocks=7")
    n_chain = max(_n_chain(rows, 1, rpi), _n_chain(rows, 7, rpi))
    _assert_pooled(one, ref, mag, n_chain, "stem_pool_bwd_reduce_out32 blocks=1")
    _assert_pooled(seven, ref, mag, n_chain, "stem_pool_bwd_reduce_out32 blocks=7")
    _assert_pooled(seven, one, mag, n_chain, "stem_pool_bwd_reduce_out32 blocks=7 against blocks=1")
