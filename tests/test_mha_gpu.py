"""Global-attention HIP kernels (csrc/kernels/mha.hip) and the converted ViT block on an MI355X.

The reference is softmax attention in fp64 from the very 16-bit q / k / v / dy the kernels read, gradients by
``torch.autograd.grad``.  Bounds are per element and derived as in tests/_numerics.py and tests/test_winattn_gpu.py
(``u = 2**-24``), nothing is tuned.  Forward, with ``l = sum_j exp(s_j - max)`` and ``blocks = ceil(N / 16)``:
    e_s  = (64 + 4) * 2u * scale * sum|q||k| + 4u * |s|                      the fp32 score, scaled once
    t    = |s - max| * log2 e + log2 l                                       the largest exponent either pass forms
    rel  = 2 * max_j e_s + (t + N + 8 + 4 * blocks) * u + 8u * (|lse| + 1)   exponential, sums, rescales, the stored lse
    e_p  = p * rel + 2**-126                                                 fp32 p (the exp2 unit flushes subnormals)
    e_pf = e_p + p * 2**-9  (bf16)  |  e_p + p * 2**-12 + 2**-25 / l  (fp16)  p rounded UNNORMALISED, divided by l later
    |o - ref|   <= sum_j e_pf |v_j| + (N + 4) * 2u * sum_j p |v_j| + half_ulp16(o)
    |lse - ref| <= max_j e_s + 8u * (|lse| + 1)                              natural domain: the kernel's lse * ln 2
Backward, P recomputed (normalised) from the stored lse, so ``e_pb = e_p + half_ulp16(p)``:
    |dv - ref| <= sum_i e_pb |dy_i| + (N + 4) * 2u * sum_i p |dy_i| + half_ulp16(dv)
    e_dp = (64 + 4) * 2u * sum_d |dy||v|                                     dP = dy v^T
    e_D  = sum_d |dy| * bound(o) + (64 + 4) * 2u * sum_d |dy||o|             delta = sum_d dy * y, y the ROUNDED output
    e_ds = e_p (|dP| + |D|) + p (e_dp + e_D) + 4u * p (|dP| + |D|)           dS = p (dP - delta)
    e_ds16 = e_ds + half_ulp16(dS)
    |dq - ref| <= scale * (sum_j e_ds16 |k_j| + (N + 4) * 2u * sum_j |dS||k_j|) + 2u |dq| + half_ulp16(dq)
    |dk - ref| <= the same over the queries with q
A single token is exact: y == v, dv == dy, dq == dk == 0.  Largest observed ratios: profiles/mha_mi355x.md.
"""
import copy
import math

import pytest
import torch

from _numerics import U, assert_within, half_ulp16

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
SCALE = 64 ** -0.5
# (B, heads, N), form, planted (query, key, sign pattern) pairs: q row = k row = +-2.0, so scale * s = 32
CASES = [
    ((2, 1, 1), "packed", ()),                       # a single token: exact
    ((3, 2, 50), "packed", ()),                      # under one key block; B * heads no multiple of anything
    ((2, 3, 64), "strided", ()),                     # exactly one full block, no masked key
    ((2, 2, 65), "packed", ((3, 64, 0),)),           # one real key in the last block, and it moves the max
    ((1, 3, 197), "packed", ((5, 196, 0), (9, 0, 1))),  # dominant key in the last block / at key 0: the max never moves
    ((1, 2, 300), "strided", ()),                    # 5 key blocks, 3 query chunks
]
_cases = lambda f: pytest.mark.parametrize("dtype", DTYPES)(
    pytest.mark.parametrize("case", CASES, ids=["x".join(map(str, c[0])) for c in CASES])(f))
_cache = {}


def _bounds(q, k, v, dy, scale, dtype):
    """The fp64 reference and the per-element bounds of the module docstring for the views ``q`` / ``k`` / ``v``
    ``[B, N, heads, 64]`` and ``dy[B, N, heads * 64]``."""
    B, N, heads, _ = q.shape
    q64, k64, v64 = (t.detach().double().permute(0, 2, 1, 3).requires_grad_(True) for t in (q, k, v))
    g64 = dy.detach().double().reshape(B, N, heads, 64).permute(0, 2, 1, 3)
    s = scale * q64 @ k64.transpose(-1, -2)
    p = torch.softmax(s, -1)
    o = p @ v64
    dq, dk, dv = torch.autograd.grad(o, (q64, k64, v64), g64)
    with torch.no_grad():
        qa, ka, va, ga = q64.abs(), k64.abs(), v64.abs(), g64.abs()
        T = lambda x: x.transpose(-1, -2)
        lse = torch.logsumexp(s, -1, keepdim=True)
        smax = s.max(-1, keepdim=True).values
        l = (lse - smax).exp()
        e_s = 68 * 2 * U * scale * (qa @ T(ka)) + 4 * U * s.abs()
        es_max = e_s.max(-1, keepdim=True).values
        t = (s - smax).abs() * math.log2(math.e) + l.log2()
        rel = 2 * es_max + (t + N + 8 + 4 * math.ceil(N / 16)) * U + 8 * U * (lse.abs() + 1)
        e_p = p * rel + 2.0 ** -126
        e_pf = e_p + (p * 2.0 ** -9 if dtype == torch.bfloat16 else p * 2.0 ** -12 + 2.0 ** -25 / l)
        e_pb = e_p + half_ulp16(p, dtype)
        acc = (N + 4) * 2 * U
        b_o = e_pf @ va + acc * (p @ va) + half_ulp16(o, dtype)
        dP = g64 @ T(v64)
        D = (p * dP).sum(-1, keepdim=True)
        dS = p * (dP - D)
        e_dp = 68 * 2 * U * (ga @ T(va))
        e_D = (ga * b_o).sum(-1, keepdim=True) + 68 * 2 * U * (ga * o.abs()).sum(-1, keepdim=True)
        e_ds = e_p * (dP.abs() + D.abs()) + p * (e_dp + e_D) + 4 * U * p * (dP.abs() + D.abs())
        e_ds16 = e_ds + half_ulp16(dS, dtype)
        tok = lambda x: x.permute(0, 2, 1, 3)  # [B, heads, N, 64] -> token-major
        ref = dict(o=tok(o), dq=tok(dq), dk=tok(dk), dv=tok(dv), lse=lse.squeeze(-1))
        bound = dict(
            o=tok(b_o), lse=(es_max + 8 * U * (lse.abs() + 1)).squeeze(-1),
            dv=tok(T(e_pb) @ ga + acc * (T(p) @ ga)) + half_ulp16(tok(dv), dtype),
            dq=tok(scale * (e_ds16 @ ka + acc * (dS.abs() @ ka)) + 2 * U * dq.abs()) + half_ulp16(tok(dq), dtype),
            dk=tok(scale * (T(e_ds16) @ qa + acc * (T(dS.abs()) @ qa)) + 2 * U * dk.abs()) + half_ulp16(tok(dk), dtype))
    return ref, bound


def _data(case, dtype):
    """Inputs on the GPU, the fp64 reference and the bounds, computed once per (case, dtype)."""
    if (case, dtype) in _cache:
        return _cache[case, dtype]
    (B, heads, N), form, planted = case
    gen = torch.Generator().manual_seed(B * 1000 + N)
    if form == "packed":
        qkv = torch.randn(B, N, 3, heads, 64, generator=gen)
    else:  # three tensors with padded token and head strides
        qkv = torch.randn(B, N + 1, 3, heads, 72, generator=gen)
    for i, j, pattern in planted:
        sign = torch.ones(64) if pattern == 0 else torch.tensor([1.0, -1.0]).repeat(32)
        qkv[:, i, 0, :, :64] = 2.0 * sign
        qkv[:, j, 1, :, :64] = 2.0 * sign
    qkv = qkv.to(dtype).to(DEV)
    if form == "packed":
        q, k, v = qkv.unbind(2)
    else:
        q, k, v = (qkv[:, :, n].contiguous()[:, :N, :, :64] for n in range(3))
        qkv = None
    dy = torch.randn(B, N, heads * 64, generator=gen).to(dtype).to(DEV)
    ref, bound = _bounds(q, k, v, dy, SCALE, dtype)
    _cache[case, dtype] = dict(q=q, k=k, v=v, qkv=qkv, dy=dy, ref=ref, bound=bound)
    return _cache[case, dtype]


def _check(got, d, k, what):
    w = assert_within(got.reshape(d["ref"][k].shape), d["ref"][k], d["bound"][k], f"{what}: {k}", family="mha_" + k)
    print(f"{what} {k}: max err / bound {w:.3e}")


_nan = lambda *shape, dtype: torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def _run(d, case, dtype):
    """Forward and backward through the raw bindings into NaN-filled outputs and workspace."""
    from pytorch_distributed_template_amd.ops import native
    (B, heads, N), form, _ = case
    y, lse = _nan(B, N, heads * 64, dtype=dtype), _nan(B, heads, N, dtype=torch.float32)
    native.C.mha_fwd(d["q"], d["k"], d["v"], y, lse, SCALE)
    if form == "packed":  # one dense dqkv
        grads = _nan(B, N, 3, heads, 64, dtype=dtype).unbind(2)
    else:
        grads = [_nan(B, N + 1, heads, 72, dtype=dtype)[:, :N, :, :64] for _ in range(3)]
    delta = _nan(B, heads, N, dtype=torch.float32)
    native.C.mha_bwd(d["dy"].view(B, N, heads, 64), y, d["q"], d["k"], d["v"], lse, *grads, delta, SCALE)
    return y, lse, grads, delta


@_cases
def test_forward(case, dtype):
    d = _data(case, dtype)
    y, lse, _, _ = _run(d, case, dtype)
    _check(y, d, "o", f"{case[0]} {dtype}")
    _check(lse.double() * math.log(2.0), d, "lse", f"{case[0]} {dtype}")
    if case[0][2] == 1:
        assert torch.equal(y.view_as(d["v"]), d["v"])


@_cases
def test_backward(case, dtype):
    d = _data(case, dtype)
    y, _, (dq, dk, dv), delta = _run(d, case, dtype)
    for k, got in (("dq", dq), ("dk", dk), ("dv", dv)):
        _check(got, d, k, f"{case[0]} {dtype}")
    assert bool(torch.isfinite(delta).all())
    if case[0][2] == 1:
        assert torch.equal(dv.reshape(d["dy"].shape), d["dy"])
        assert not bool(dq.any()) and not bool(dk.any())


@pytest.mark.parametrize("dtype", DTYPES)
def test_bit_identical(dtype):
    d = _data(CASES[4], dtype)
    a, b = _run(d, CASES[4], dtype), _run(d, CASES[4], dtype)
    for x, y in zip((a[0], a[1], *a[2], a[3]), (b[0], b[1], *b[2], b[3])):
        assert torch.equal(x, y)


@pytest.mark.parametrize("dtype", DTYPES)
def test_autograd_function(dtype):
    from pytorch_distributed_template_amd.ops import mha
    (B, heads, N), _, _ = case = CASES[4]
    d = _data(case, dtype)
    qkv = d["qkv"].reshape(B, N, 3 * heads * 64).clone().requires_grad_(True)
    y = mha._PackedFn.apply(qkv, heads, SCALE)
    y.backward(d["dy"])
    for k, got in zip(("o", "dq", "dk", "dv"), (y, *qkv.grad.view(B, N, 3, heads, 64).unbind(2))):
        _check(got, d, k, f"function {dtype}")


def test_operand_strides():
    from pytorch_distributed_template_amd.ops import mha
    d = _data(CASES[1], torch.bfloat16)
    y, lse = mha.mha_attention_fwd(d["q"], d["k"], d["v"], SCALE)
    out = [torch.empty(1, 1, 1, 64, dtype=torch.bfloat16, device=DEV).expand(3, 50, 2, 64) for _ in range(3)]
    before = _counts()
    with pytest.raises(RuntimeError, match="positive"):  # an overlapping output view: refused before any launch
        mha.mha_attention_bwd(d["dy"], y, d["q"], d["k"], d["v"], lse, SCALE, out=out)
    assert _counts() == before


def _counts():
    from pytorch_distributed_template_amd.ops import native
    c = native.C.dispatch_counts()
    return [c.get(k, 0) for k in ("mha_fwd", "mha_bwd")]


def test_converted_module_trains():
    """One training step of a ViT block under bf16 autocast.  The attention it ran is read off the autograd node of the
    y handed to ``out_proj`` and held to the derived bounds; behind the bf16 Linears no bound is derived, none asserted"""
    from pytorch_distributed_template_amd.models import modern
    from pytorch_distributed_template_amd.ops import mha
    torch.manual_seed(3)
    block = modern.EncoderBlock(2, 128, 256, 0.0, 0.0).to(DEV).train()
    with torch.no_grad():
        block.self_attention.in_proj_weight.mul_(4.0)  # scores that matter
    stock = copy.deepcopy(block.self_attention)
    assert mha.convert_mha(block) == 1
    attn, seen = block.self_attention, {}

    def grab(_, inputs):  # out_proj's input is the attention's y: its autograd node holds the rest
        node = inputs[0].grad_fn
        seen.update(y=inputs[0].detach(), saved=node.saved_tensors, scale=node.scale)
        node.register_hook(lambda gin, gout: seen.update(gin=gin, dy=gout[0]))

    handle = attn.out_proj.register_forward_pre_hook(grab)
    x = torch.randn(3, 50, 128, device=DEV)
    before = _counts()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = block(x)
    out.backward(torch.randn_like(out))
    assert [a - b for a, b in zip(_counts(), before)] == [1, 1]
    handle.remove()

    qkv, y, lse = seen["saved"]
    assert qkv.shape == (3, 50, 384) and qkv.dtype == torch.bfloat16 and seen["scale"] == 0.125
    q, k, v = qkv.view(3, 50, 3, 2, 64).unbind(2)
    ref, bound = _bounds(q, k, v, seen["dy"], 0.125, torch.bfloat16)
    for name, got in zip(("o", "dq", "dk", "dv"), (seen["y"], *seen["gin"][0].view(3, 50, 3, 2, 64).unbind(2))):
        w = assert_within(got.reshape(ref[name].shape), ref[name], bound[name], f"module: {name}",
                          family="mha_module_" + name)
        print(f"module {name}: max err / bound {w:.3e}")

    before = _counts()  # what the kernels do not cover goes to the parent, unchanged
    mask = torch.zeros(50, 50, device=DEV)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        for kw in (dict(need_weights=True), dict(need_weights=False, attn_mask=mask)):
            got, want = attn(x, x, x, **kw), stock(x, x, x, **kw)
            assert torch.equal(got[0], want[0]) and (want[1] is None or torch.equal(got[1], want[1]))
    assert _counts() == before
