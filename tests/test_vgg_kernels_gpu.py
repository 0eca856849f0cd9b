"""The VGG-family kernels of vgg.hip per element against fp64, in bf16 and fp16: bn_relu_maxpool2, maxpool2_bwd (BN and
bias forms), fc_act_fwd / fc_act_bwd (bias + ReLU + dropout), and the pooled reduce fed with bn_relu_maxpool2's output.

References, bounds and assertions are those of tests/_pool_cases.py (derived there; proved on the CPU in
tests/test_numerics_model_cpu.py).  Differences from the 3x3 pool: an exact tie goes to the lowest scan position
k = dh * 2 + dw, and there is no dead code -- a window without a positive member gives out = 0, idx = 0.

maxpool2_bwd is judged on inputs whose argmax is decisive in every window (``pc.make_decisive`` redraws, on the CPU,
every window whose two largest fp64 values are closer than twice the bound, or whose maximum a 16-bit rounding could take
to zero): the fp64 dz is then unique and does not depend on the kernel's idx.  The BN form rounds A*dz + B*y + Cc once:
half_ulp16(ref) + 8u * mag; the bias form copies: dy equals dz bit for bit.

fc_act_fwd adds the fp32 bias (one correctly rounded fp32 addition), multiplies the kept elements by the fp32
``1 / (1 - p)`` (one fp32 rounding) and rounds to 16 bits: every step is reproduced exactly through fp64, so both
directions are compared bit for bit.  The keep decision is ``vgg_hash(seed, i) >= thr``; the tests reimplement the
documented 64-bit mix and pin the dropout stream on purpose.

Output buffers start as NaN, argmax buffers as 0x77 (a byte no kernel writes).
"""
import numpy as np
import pytest
import torch

import _conv_cases as cc
import _numerics as nm
import _pool_cases as pc

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = cc.DTYPES
UNWRITTEN = 0x77
# (N, H, W, C): the shape of the older test; one window per image and one vector per pixel; C = 8 with a 3 x 2 pooled map;
# VGG's widest layer; a width that is no multiple of 16 over an odd pooled side
POOL2_SHAPES = [(3, 12, 10, 64), (2, 2, 2, 8), (1, 6, 4, 8), (2, 4, 6, 512), (5, 14, 14, 24)]
FC_SHAPES = [(64, 4096), (1, 8), (37, 136)]
GRID_VECTORS = 65536 * 256  # vgg.hip's kEwCap blocks of 256 threads: one full grid-stride pass


def _C():
    from pytorch_distributed_template_amd.ops import native
    return native.C


def _nan(*shape, dtype):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def _idxbuf(*shape):
    return torch.full(shape, UNWRITTEN, dtype=torch.uint8, device=DEV)


def _fam(name, dtype):
    return f"{name}_{'bf16' if dtype == torch.bfloat16 else 'fp16'}"


def _dev(d):
    return {k: (v.to(DEV).contiguous() if torch.is_tensor(v) else v) for k, v in d.items()}


def _bias_form(d, C):
    """Replace the hand-made [1 | b | 0 | 1] by the block bias_coef writes, after holding them equal."""
    coef = _nan(4 * C, dtype=torch.float32)
    _C().bias_coef(d["coef"][C:2 * C].contiguous(), coef, C)
    assert torch.equal(coef, d["coef"])
    return dict(d, coef=coef)


def _pool2(d, N, H, W, C, dtype, with_idx=True):
    out = _nan(N, H // 2, W // 2, C, dtype=dtype)
    idx = _idxbuf(N, H // 2, W // 2, C) if with_idx else None
    _C().bn_relu_maxpool2(d["y"], d["coef"], out, idx, N, H, W, C)
    return out, idx


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form,layer", [("bn", "real"), ("bn", "int"), ("bias", "real")])
@pytest.mark.parametrize("N,H,W,C", POOL2_SHAPES)
def test_bn_relu_maxpool2(N, H, W, C, form, layer, dtype):
    """out and idx by the rules of _pool_cases (``int``: out exact and, every window being decisive or dead, every
    argmax byte pinned -- the four integer values of a window tie often: the lowest scan position wins); the eval form
    (idx = None) writes the same out."""
    d = _dev(pc.pool2_operands(N, H, W, C, layer, dtype, form))
    if form == "bias":
        d = _bias_form(d, C)
    r = pc.pool_fwd_ref(d["y"], d["coef"], 2, 0)
    if layer == "int":
        assert bool((r["decisive"] | r["must_dead"]).all())
    out, idx = _pool2(d, N, H, W, C, dtype)
    name = f"bn_relu_maxpool2 {form} {layer} {dtype}"
    pc.assert_pool_fwd(out, idx, r, dtype, None, name, _fam("pool2_fwd", dtype), exact=layer == "int")
    out_eval, _ = _pool2(d, N, H, W, C, dtype, with_idx=False)
    assert torch.equal(out_eval.view(torch.int16), out.view(torch.int16)), f"{name}: the eval form writes another out"


@pytest.mark.parametrize("dtype", DTYPES)
def test_bn_relu_maxpool2_constant_windows_tie_to_position_0(dtype):
    """Every window holds one value four times (positive and negative pre-activations): idx = 0 everywhere, and the
    backward routes the gradient to position 0 alone."""
    N, H, W, C = 2, 6, 8, 16
    d = pc.pool2_operands(N, H, W, C, "real", dtype)
    d["y"] = d["y"][:, ::2, ::2].repeat_interleave(2, 1).repeat_interleave(2, 2).contiguous()
    d = _dev(d)
    r = pc.pool_fwd_ref(d["y"], d["coef"], 2, 0)
    assert bool((r["first"] == 0).all()) and bool((r["ref"] > 0).any()) and bool((r["ref"] == 0).any())
    out, idx = _pool2(d, N, H, W, C, dtype)
    pc.assert_pool_fwd(out, idx, r, dtype, None, f"bn_relu_maxpool2 ties {dtype}", _fam("pool2_fwd", dtype))
    assert not bool(idx.any()), "a tie did not go to scan position 0"
    dy = _nan(N, H, W, C, dtype=dtype)
    _C().maxpool2_bwd(d["dp"], idx, out, d["y"], d["b"], dy, N, H, W, C)
    _, ref, mag = pc.pool2_bwd_ref(d, r, mask=out.double() > 0)
    nm.assert_rounded(dy, ref, mag, dtype, name=f"maxpool2_bwd ties {dtype}", C=C, family=_fam("pool2_bwd", dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form,layer", [("bn", "real"), ("bn", "int"), ("bias", "real")])
@pytest.mark.parametrize("N,H,W,C", POOL2_SHAPES)
def test_maxpool2_bwd(N, H, W, C, form, layer, dtype):
    """Forward kernel, then backward kernel on its out / idx, against the fp64 dz of decisive inputs (unique, so
    independent of the kernel's idx); then the scatter alone along random argmax bytes 0..3 and a random mask."""
    d = pc.pool2_operands(N, H, W, C, layer, dtype, form)
    d["y"] = pc.make_decisive(d["y"], d["coef"], dtype, 2, 0, seed=H * W + C)
    d = _dev(d)
    if form == "bias":
        d = _bias_form(d, C)
    r = pc.pool_fwd_ref(d["y"], d["coef"], 2, 0)
    assert bool(pc.settled(r).all()) and bool((r["ref"] > 0).any())
    out, idx = _pool2(d, N, H, W, C, dtype)
    name = f"maxpool2_bwd {form} {layer} {dtype}"
    pc.assert_pool_fwd(out, idx, r, dtype, None, name + ": forward", exact=layer == "int")
    assert torch.equal(idx.long(), r["first"]) and torch.equal(out.double() > 0, r["ref"] > 0)
    y, b = (d["y"], d["b"]) if form == "bn" else (None, None)

    def check(idx_, out_, dz, ref, mag, what):
        dy = _nan(N, H, W, C, dtype=dtype)
        _C().maxpool2_bwd(d["dp"], idx_, out_, y, b, dy, N, H, W, C)
        if form == "bias":  # a copy: dz itself, bit for bit
            nm.assert_exact(dy, dz, f"{name}: {what}")
        elif layer == "int":
            nm.assert_exact(dy, nm.round_exact(ref, dtype), f"{name}: {what}")
        else:
            nm.assert_rounded(dy, ref, mag, dtype, name=f"{name}: {what}", C=C, family=_fam("pool2_bwd", dtype))

    check(idx, out, *pc.pool2_bwd_ref(d, r), "dy")
    g = torch.Generator().manual_seed(H + W + C)
    ridx = torch.randint(0, 4, idx.shape, generator=g, dtype=torch.uint8).to(DEV)
    rout = torch.where(torch.rand(idx.shape, generator=g).to(DEV) < 0.7, out.abs() + 1, torch.zeros_like(out))
    check(ridx, rout, *pc.pool2_bwd_ref(d, r, pos=ridx, mask=rout.double() > 0), "scatter along given bytes")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,H,W,C", [(3, 12, 10, 64), (5, 14, 14, 24)])
def test_pooled_reduce_matches_the_true_y_at_the_argmax_2x2(N, H, W, C, dtype):
    """pooled_bwd_reduce on bn_relu_maxpool2's out: the sums agree with those over the true y at the argmax within the
    formula bound plus the rounding of out carried into xhat (this replaces an rtol / atol = 2e-2 comparison)."""
    C_ = _C()
    S = C_.stat_slots()
    d = _dev(pc.pool2_operands(N, H, W, C, "real", dtype, seed=5))
    out, idx = _pool2(d, N, H, W, C, dtype)
    ref, mag, carry = pc.pooled_link_ref(d["y"], d["coef"], d["dp"], idx, out, 2, 0, dtype)
    rows = out.numel() // C
    n_chain = pc.reduce16_plan(rows, C, 2048)[2]
    slots = _nan(S * C * 2, dtype=torch.float64)
    C_.pooled_bwd_reduce(d["dp"], out, d["coef"], slots, rows, C)
    assert bool(torch.isfinite(slots).all())
    pc.assert_pooled_link(slots.view(S, C, 2).sum(0), ref, mag, carry, n_chain, f"pooled_bwd_reduce 2x2 {dtype}",
                          _fam("pool16_reduce_link", dtype))


# ------------------------------------------------------------------------------------------------ classifier
def _fc_operands(rows, F_, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(rows, F_, generator=g).to(dtype).to(DEV)
    bias = (torch.randn(F_, generator=g) * 0.5).to(DEV)
    dh = torch.randn(rows, F_, generator=g).to(dtype).to(DEV)
    return z, bias, dh


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,F_", FC_SHAPES)
@pytest.mark.parametrize("p,seed", [(0.0, 0), (0.5, 0), (0.5, 11), (0.1, 2 ** 63 - 1), (2.0 ** -33, 11), (0.999, 11)])
def test_fc_act_fwd_and_bwd(p, seed, rows, F_, dtype):
    """Bit for bit: out = round(relu(z + b) * scale) on the kept set {i: hash(seed, i) >= thr} (p = 0: everywhere) and
    dz = round(dh * scale) where out > 0.  p = 2**-33 clamps thr to 1; seeds up to 2**63 - 1."""
    z, bias, dh = _fc_operands(rows, F_, dtype, rows + F_)
    thr, scale = pc.dropout_consts(p)
    keep = None
    if p > 0:
        keep = torch.from_numpy(pc.vgg_hash_np(seed, rows * F_) >= np.uint32(thr)).to(DEV)
        if p == 0.5 and rows * F_ > 1000:
            assert 0.45 < float(keep.double().mean()) < 0.55
    out = _nan(rows, F_, dtype=dtype)
    _C().fc_act_fwd(z, bias, out, rows, F_, p, seed)
    expect = pc.fc_act_ref(z, bias, F_, p, keep, dtype)
    name = f"fc_act_fwd p={p} seed={seed} {dtype}"
    if keep is not None:  # the kept set, element for element, wherever the kept value is visible
        seen = pc.fc_act_ref(z, bias, F_, p, None, dtype) > 0
        bad = ((out.double() > 0) != (keep.view(rows, F_) & seen)).nonzero()
        assert bad.numel() == 0, f"{name}: {bad.shape[0]} keep decisions differ; first at {tuple(bad[0].tolist())}"
    nm.assert_exact(out, expect, name)
    dz = _nan(rows, F_, dtype=dtype)
    _C().fc_act_bwd(dh, out, dz, p)
    nm.assert_exact(dz, pc.fc_act_bwd_ref(dh, out, p, dtype), f"fc_act_bwd p={p} {dtype}")


# ------------------------------------------------------------------------------------------------ second grid pass
def test_fc_act_second_grid_stride_pass():
    """One 8-element vector more than a full grid (65536 blocks of 256 threads): the last vector is written by the second
    pass of thread 0, with the bias of its own feature group and the hash of its own element index.  The reference is
    computed on the GPU in 16-bit / int64 chunks (``pc.vgg_hash_torch``; no fp64 copy of the tensors)."""
    dtype, F_ = torch.bfloat16, 776  # 97 vectors per row; 97 * 172961 == 2**24 + 1
    rows = (GRID_VECTORS + 1) // (F_ // 8)
    assert rows * (F_ // 8) == GRID_VECTORS + 1
    p, seed = 0.5, 11
    thr, scale = pc.dropout_consts(p)
    g = torch.Generator(device=DEV).manual_seed(3)
    z = torch.randn(rows, F_, device=DEV, generator=g).to(dtype)
    bias = torch.randn(F_, device=DEV, generator=g) * 0.5
    out = _nan(rows, F_, dtype=dtype)
    _C().fc_act_fwd(z, bias, out, rows, F_, p, seed)
    dz = _nan(rows, F_, dtype=dtype)
    _C().fc_act_bwd(z, out, dz, p)  # z stands in for dh
    step = 8192
    nbad = 0
    for lo in range(0, rows, step):
        hi = min(rows, lo + step)
        keep = (pc.vgg_hash_torch(seed, (hi - lo) * F_, lo * F_, DEV) >= thr).view(hi - lo, F_)
        # fp32 sum, fp32 product with the scale 2 (exact), one rounding: the kernel's own steps in torch's fp32
        val = torch.where(keep, torch.relu(z[lo:hi].float() + bias) * scale, torch.zeros((), device=DEV)).to(dtype)
        nbad += int((val.view(torch.int16) != out[lo:hi].view(torch.int16)).sum())
        dzr = torch.where(out[lo:hi] > 0, z[lo:hi].float() * scale, torch.zeros((), device=DEV)).to(dtype)
        nbad += int((dzr.view(torch.int16) != dz[lo:hi].view(torch.int16)).sum())
    last = pc.fc_act_ref(z[-1:], bias, F_, p, torch.from_numpy(
        pc.vgg_hash_np(seed, F_, (rows - 1) * F_) >= np.uint32(thr)).to(DEV), dtype)
    nm.assert_exact(out[-1:], last, "fc_act_fwd: the last row against the numpy hash")
    del z, out, dz
    torch.cuda.empty_cache()
    assert nbad == 0, f"fc_act second pass: {nbad} elements differ from the exact 16-bit reference"


def test_maxpool2_second_grid_stride_pass():
    """bn_relu_maxpool2 / maxpool2_bwd in the bias form with scale 1 and shift 0 over 2**24 + 1 pooled vectors: out is
    the exact 16-bit maximum of relu(y), idx the first position holding it, dy the exact scatter -- all computed on the
    GPU from strided 16-bit views."""
    dtype, C = torch.bfloat16, 8
    N, OH, OW = 97, 257, 673  # 97 * 257 * 673 == 2**24 + 1 vectors of 8 channels
    assert N * OH * OW == GRID_VECTORS + 1
    H, W = 2 * OH, 2 * OW
    g = torch.Generator(device=DEV).manual_seed(4)
    y = torch.empty(N, H, W, C, device=DEV, dtype=dtype)
    for n in range(N):
        y[n] = torch.randn(H, W, C, device=DEV, generator=g).to(dtype)
    dp = torch.randn(N, OH, OW, C, device=DEV, generator=g).to(dtype)
    coef = torch.cat([torch.ones(C), torch.zeros(2 * C), torch.ones(C)]).to(DEV)
    out, idx = _nan(N, OH, OW, C, dtype=dtype), _idxbuf(N, OH, OW, C)
    _C().bn_relu_maxpool2(y, coef, out, idx, N, H, W, C)
    dy = _nan(N, H, W, C, dtype=dtype)
    _C().maxpool2_bwd(dp, idx, out, None, None, dy, N, H, W, C)
    zero = torch.zeros((), device=DEV, dtype=dtype)
    members = [torch.relu(y[:, k >> 1::2, k & 1::2]) for k in range(4)]
    best = torch.maximum(torch.maximum(members[0], members[1]), torch.maximum(members[2], members[3]))
    first = torch.full(best.shape, 4, device=DEV, dtype=torch.uint8)
    for k in (3, 2, 1, 0):
        first = torch.where(members[k] == best, torch.full_like(first, k), first)
    bad_out = int((out != best).sum())
    bad_idx = int((idx != first).sum())
    gz = torch.where(best > 0, dp, zero)
    bad_dy = sum(int((dy[:, k >> 1::2, k & 1::2] != torch.where(first == k, gz, zero)).sum()) for k in range(4))
    del y, dy, members, best, first, gz, out, idx, dp
    torch.cuda.empty_cache()
    assert (bad_out, bad_idx, bad_dy) == (0, 0, 0), f"second pass: {bad_out} out, {bad_idx} idx, {bad_dy} dy elements differ"
