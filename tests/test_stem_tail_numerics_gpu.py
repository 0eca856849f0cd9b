"""The 16-bit pooling kernels and stem tail of pool.hip per element against fp64, in bf16 and fp16: bn_relu_maxpool
(pad 1: the ResNet stem, pad 0: AlexNet), maxpool_bwd_relu, stem_pool_bwd_apply, stem_pool_bwd_reduce and the pooled
reduce (stem_pool_bwd_reduce_out / pooled_bwd_reduce) fed with bn_relu_maxpool's own output.

Every reference is fp64 from the very 16-bit / fp32 values the kernel reads and independent of every other kernel here
(the pooled reduce's semantic link alone takes ``out`` and ``idx`` from bn_relu_maxpool: that link is what it checks).
The bounds, their derivation and the assertions live in tests/_pool_cases.py; tests/test_numerics_model_cpu.py proves
them on the CPU.  Two layers as in tests/test_conv_numerics_gpu.py: ``int`` (integer operands, power-of-two
coefficients: bit-exact) and ``real`` (bounded).  Output buffers start as NaN, argmax buffers as 0x77, a byte no kernel
writes (window positions are 0..8, the dead code is 255).

The argmax operands of the backward kernels (``cc.stem_tail_operands``) are random bytes 0..8 -- at pad 1 some point
outside the image --, a tenth of them the dead code 255; the reference routes nothing from either.
"""
import pytest
import torch

import _conv_cases as cc
import _numerics as nm
import _pool_cases as pc

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = cc.DTYPES
LAYERS = ["int", "real"]
UNWRITTEN = 0x77
# (pad, N, H, W, C): odd and even sides (border windows of 4 and 6 members; at pad 0 an even side leaves a last row /
# column no window covers), one vector per pixel (C = 8), a single window, AlexNet's 27 x 27 x 192 (more than one block)
POOL_SHAPES = [(1, 2, 12, 11, 64), (1, 2, 13, 11, 8), (0, 2, 13, 11, 64), (0, 2, 12, 10, 8), (0, 1, 3, 3, 8),
               (0, 1, 4, 4, 16), (0, 3, 27, 27, 192)]
TAIL_SHAPES = [(2, 12, 11, 64), (2, 13, 11, 64), (2, 55, 55, 64), (1, 3, 5, 64)]


def _C():
    from pytorch_distributed_template_amd.ops import native
    return native.C


def _fam(name, dtype):
    return f"{name}_{'bf16' if dtype == torch.bfloat16 else 'fp16'}"


def _nan(*shape, dtype):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def _idxbuf(*shape):
    return torch.full(shape, UNWRITTEN, dtype=torch.uint8, device=DEV)


def _operands(N, H, W, layer, dtype, C, pad=1, seed=0):
    return {k: v.to(DEV).contiguous() for k, v in cc.stem_tail_operands(N, H, W, layer, dtype, C=C, seed=seed,
                                                                        pad=pad).items()}


def _pool(y, coef, N, H, W, C, pad, dtype):
    OH, OW = pc.out_hw(H, W, 3, pad)
    out, idx = _nan(N, OH, OW, C, dtype=dtype), _idxbuf(N, OH, OW, C)
    _C().bn_relu_maxpool(y, coef, out, idx, N, H, W, C, pad=pad)
    return out, idx


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("pad,N,H,W,C", POOL_SHAPES)
def test_bn_relu_maxpool16(pad, N, H, W, C, dtype):
    """out within half_ulp16(ref) + 8u * mag of the fp64 window maximum; idx by the rules of _pool_cases (255 required /
    forbidden, in-image, value within the bound, the fp64 argmax where the window is decisive).  BN scales of mixed
    sign; channel 1 at 1e-3."""
    d = _operands(N, H, W, "real", dtype, C, pad)
    out, idx = _pool(d["y"], d["coef"], N, H, W, C, pad, dtype)
    r = pc.pool_fwd_ref(d["y"], d["coef"], 3, pad)
    pc.assert_pool_fwd(out, idx, r, dtype, 255, f"bn_relu_maxpool pad={pad} {dtype}", family=_fam("pool16_fwd", dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("pad,N,H,W,C", POOL_SHAPES)
def test_bn_relu_maxpool16_decisive(pad, N, H, W, C, dtype):
    """The integer planes of test_bn_relu_maxpool32_decisive: every window is decisive or all-negative, so out (exact)
    and every argmax byte (the fp64 argmax, or 255 for the all-negative planes c % 8 == 5) are pinned."""
    y, coef = pc.decisive_planes(N, H, W, C, H + C + pad)
    y, coef = y.to(dtype).to(DEV), coef.to(DEV)
    out, idx = _pool(y, coef, N, H, W, C, pad, dtype)
    r = pc.pool_fwd_ref(y, coef, 3, pad)
    assert bool((r["decisive"] | r["must_dead"]).all()) and bool(r["must_dead"][..., 5].all())
    assert bool(r["decisive"].any())
    pc.assert_pool_fwd(out, idx, r, dtype, 255, f"bn_relu_maxpool decisive pad={pad} {dtype}", exact=True)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layer", LAYERS)
@pytest.mark.parametrize("pad,N,H,W,C", POOL_SHAPES)
def test_maxpool_bwd_relu16(pad, N, H, W, C, layer, dtype):
    """dz against the fp64 scatter of dp along the given argmax bytes with the ReLU mask from y (``int``: exact).  At
    pad 0 an even side has a last row / column that no window covers: exact zeros."""
    d = _operands(N, H, W, layer, dtype, C, pad)
    r = cc.stem_tail_ref(d, N, H, W, C, pad)
    dz = _nan(N, H, W, C, dtype=dtype)
    _C().maxpool_bwd_relu(d["dp"], d["idx"], d["y"], d["coef"], dz, N, H, W, C, pad=pad)
    _, share = pc.assert_pool_bwd(dz, r, dtype, f"maxpool_bwd_relu pad={pad} {layer} {dtype}", _fam("pool16_bwd", dtype),
                                  exact=layer == "int")
    assert share > 0.99
    if pad == 0:
        OH, OW = pc.out_hw(H, W, 3, 0)
        if 2 * OH + 1 < H:
            assert float(r["dzmag"][:, 2 * OH + 1:].abs().max()) == 0.0 and not bool(dz[:, 2 * OH + 1:].any())
        if 2 * OW + 1 < W:
            assert float(r["dzmag"][:, :, 2 * OW + 1:].abs().max()) == 0.0 and not bool(dz[:, :, 2 * OW + 1:].any())
    assert bool(r["dz"].any())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layer", LAYERS)
@pytest.mark.parametrize("N,H,W,C", TAIL_SHAPES)
def test_stem_pool_bwd_apply16(N, H, W, C, layer, dtype):
    """dY = A*dz + B*y + Cc with dz gathered in the kernel: half_ulp16(ref) + 12u * dymag (``int``: exact)."""
    d = _operands(N, H, W, layer, dtype, C)
    r = cc.stem_tail_ref(d, N, H, W, C)
    ref, _ = nm.bn_bwd_apply_ref(r["dz"], d["y"], d["b"], C)
    assert float((ref.view_as(r["dy"]) - r["dy"]).abs().max()) == 0.0
    dy = _nan(N, H, W, C, dtype=dtype)
    _C().stem_pool_bwd_apply(d["dp"], d["idx"], d["y"], d["coef"], d["b"], dy, N, H, W, C)
    _, share = pc.assert_tail_apply(dy, r, dtype, f"stem_pool_bwd_apply {layer} {dtype}", _fam("stem16_tail_apply", dtype),
                                    exact=layer == "int")
    assert share > 0.99


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layer", LAYERS)
@pytest.mark.parametrize("N,H,W,C", TAIL_SHAPES + [(2, 13, 11, 8)])
def test_stem_pool_bwd_reduce16(N, H, W, C, layer, dtype):
    """sum dz and sum dz * xhat against the same independent fp64 dz, chain length from the kernel's lane plan
    (col_plan(rows, C, 8, 2, 8, 4096) over the pooled pixels); unsure pixels enter the bound (``int``: exact)."""
    C_ = _C()
    S = C_.stat_slots()
    d = _operands(N, H, W, layer, dtype, C, seed=3)
    r = cc.stem_tail_ref(d, N, H, W, C)
    OH, OW = pc.out_hw(H, W, 3, 1)
    _, _, n_chain = pc.reduce16_plan(N * OH * OW, C, 4096)
    slots = _nan(S * C * 2, dtype=torch.float64)
    C_.stem_pool_bwd_reduce(d["dp"], d["idx"], d["y"], d["coef"], slots, N, H, W, C)
    assert bool(torch.isfinite(slots).all())
    got = slots.view(S, C, 2).sum(0)
    pc.assert_tail_reduce(got, d, r, C, n_chain, f"stem_pool_bwd_reduce {layer} {dtype}", _fam("stem16_tail_reduce", dtype),
                          exact=layer == "int")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("pad,N,H,W,C", [(1, 2, 12, 11, 64), (1, 2, 13, 11, 8), (0, 2, 13, 11, 64), (0, 3, 27, 27, 192)])
def test_pooled_reduce_matches_the_true_y_at_the_argmax(pad, N, H, W, C, dtype):
    """The semantic link of the pooled reduce: with ``out`` and ``idx`` from bn_relu_maxpool, the sums it recovers from
    the pooled tensors alone agree with the sums over the true y at the argmax within the formula bound plus the 16-bit
    rounding of ``out`` carried into xhat.  Pad 1 runs stem_pool_bwd_reduce_out, pad 0 pooled_bwd_reduce (one kernel)."""
    C_ = _C()
    S = C_.stat_slots()
    d = _operands(N, H, W, "real", dtype, C, pad, seed=5)
    out, idx = _pool(d["y"], d["coef"], N, H, W, C, pad, dtype)
    ref, mag, carry = pc.pooled_link_ref(d["y"], d["coef"], d["dp"], idx, out, 3, pad, dtype)
    rows = out.numel() // C
    _, _, n_chain = pc.reduce16_plan(rows, C, 2048)
    slots = _nan(S * C * 2, dtype=torch.float64)
    if pad == 1:
        C_.stem_pool_bwd_reduce_out(d["dp"], out, d["coef"], slots, N, H, W, C)
    else:
        C_.pooled_bwd_reduce(d["dp"], out, d["coef"], slots, rows, C)
    assert bool(torch.isfinite(slots).all())
    pc.assert_pooled_link(slots.view(S, C, 2).sum(0), ref, mag, carry, n_chain, f"pooled reduce pad={pad} {dtype}",
                          _fam("pool16_reduce_link", dtype))
