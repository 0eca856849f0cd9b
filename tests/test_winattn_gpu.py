"""Window attention HIP kernels (csrc/kernels/winattn.hip) and the converted Swin / MaxViT modules on an MI355X.

The reference is softmax attention written out in fp64 from the very 16-bit q / k / v / dy and fp32 bias the kernels
read, its gradients by ``torch.autograd.grad``.  Bounds are per element, in the manner of tests/_numerics.py
(``u = 2**-24``; an fp32 accumulation of n terms costs ``(n + 4) * 2u * mag``), nothing is tuned.  Forward:

    e_s  = (32 + 4) * 2u * scale * sum|q||k| + 4u * (|s| + |bias|)          the fp32 score
    rel  = 2 * max_j e_s + (|t| + N + 8) * u,  t = (s - max) * log2 e       exponential and normalisation
    e_p  = p * rel + 2**-126                                                 fp32 p (the exp2 unit flushes subnormals)
    e_p16 = e_p + half_ulp16(p)                                              p as an MFMA operand
    |o - ref| <= sum_j e_p16 |v_j| + (N + 4) * 2u * sum_j p |v_j| + half_ulp16(o)

Backward, with P recomputed from the saved row max / sum by the same arithmetic (so e_p, e_p16 as above):

    |dv - ref| <= sum_i e_p16 |dy_i| + (N + 4) * 2u * sum_i p |dy_i| + half_ulp16(dv)
    e_dp = (32 + 4) * 2u * sum_d |dy||v|                                     dP = dy v^T
    e_D  = sum_j (e_p |dP| + p e_dp) + (N + 4) * 2u * sum_j p |dP|           D = sum_j p dP
    e_ds = e_p (|dP| + |D|) + p (e_dp + e_D) + 4u * p (|dP| + |D|)           dS = p (dP - D): cancellation by magnitudes
    e_ds16 = e_ds + half_ulp16(dS)
    |dq - ref| <= scale * (sum_j e_ds16 |k_j| + (N + 4) * 2u * sum_j |dS||k_j|) + 2u |dq| + half_ulp16(dq)
    |dk - ref| <= the same over the queries with q
    |dbias - ref| <= sum_w e_ds + (Bw + 4) * 2u * sum_w |dS|                 unrounded dS, an fp32 sum of Bw terms

Largest observed ratios: profiles/winattn_mi355x.md.
"""
import pytest
import torch

from _numerics import U, assert_within, half_ulp16

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
LOG2E = 1.4426950408889634
# (Bw, nwin, heads, N), form, scale, max_blocks
CASES = [
    ((3, 0, 1, 49), "packed", 32 ** -0.5, None),    # no region; one head; windows no multiple of the waves; the +30 row
    ((8, 4, 3, 49), "separate", 1.0, None),         # all nine label classes; Bw = 2 nwin; strided q / k / v
    ((5, 0, 2, 64), "packed", 1.0, None),           # full tile, no masked keys
    ((6, 2, 3, 9), "separate", 32 ** -0.5, None),   # most of the tile masked
    ((300, 4, 3, 49), "packed", 32 ** -0.5, 6),     # 8 window slots: 38 windows per wave, 8 dbias slabs
]
_cache = {}


def _bounds(q, k, v, dy, bias, region, scale, dtype):
    """The fp64 reference and the per-element bounds of the module docstring for the views ``q`` / ``k`` / ``v``
    ``[Bw, N, heads, 32]``, ``dy[Bw, N, heads * 32]``, the fp32 ``bias`` and the uint8 ``region`` (or None)."""
    Bw, N, heads, _ = q.shape
    q64, k64, v64 = (t.detach().double().permute(0, 2, 1, 3).requires_grad_(True) for t in (q, k, v))
    b64 = bias.detach().double().requires_grad_(True)
    g64 = dy.detach().double().reshape(Bw, N, heads, 32).permute(0, 2, 1, 3)
    s = scale * q64 @ k64.transpose(-1, -2) + b64
    if region is not None:
        lab = region[torch.arange(Bw, device=DEV) % region.shape[0]].long()
        s = s + (lab[:, None, :, None] != lab[:, None, None, :]).double() * -100.0
    p = torch.softmax(s, -1)
    o = p @ v64
    dq, dk, dv, db = torch.autograd.grad(o, (q64, k64, v64, b64), g64)
    with torch.no_grad():
        qa, ka, va, ga = q64.abs(), k64.abs(), v64.abs(), g64.abs()
        e_s = 36 * 2 * U * scale * (qa @ ka.transpose(-1, -2)) + 4 * U * (s.abs() + b64.abs())
        t = (s - s.max(-1, keepdim=True).values) * LOG2E
        e_p = p * (2 * e_s.max(-1, keepdim=True).values + (t.abs() + N + 8) * U) + 2.0 ** -126
        e_p16 = e_p + half_ulp16(p, dtype)
        acc = (N + 4) * 2 * U
        dP = g64 @ v64.transpose(-1, -2)
        D = (p * dP).sum(-1, keepdim=True)
        dS = p * (dP - D)
        e_dp = 36 * 2 * U * (ga @ va.transpose(-1, -2))
        e_D = (e_p * dP.abs() + p * e_dp).sum(-1, keepdim=True) + acc * (p * dP.abs()).sum(-1, keepdim=True)
        e_ds = e_p * (dP.abs() + D.abs()) + p * (e_dp + e_D) + 4 * U * p * (dP.abs() + D.abs())
        e_ds16 = e_ds + half_ulp16(dS, dtype)
        tok = lambda x: x.permute(0, 2, 1, 3)  # [Bw, heads, N, 32] -> token-major
        ref = dict(o=tok(o), dq=tok(dq), dk=tok(dk), dv=tok(dv), db=db)
        bound = dict(
            o=tok(e_p16 @ va + acc * (p @ va)) + half_ulp16(tok(o), dtype),
            dv=tok(e_p16.transpose(-1, -2) @ ga + acc * (p.transpose(-1, -2) @ ga)) + half_ulp16(tok(dv), dtype),
            dq=tok(scale * (e_ds16 @ ka + acc * (dS.abs() @ ka)) + 2 * U * dq.abs()) + half_ulp16(tok(dq), dtype),
            dk=tok(scale * (e_ds16.transpose(-1, -2) @ qa + acc * (dS.abs().transpose(-1, -2) @ qa)) + 2 * U * dk.abs())
            + half_ulp16(tok(dk), dtype),
            db=e_ds.sum(0) + (Bw + 4) * 2 * U * dS.abs().sum(0))
    return ref, bound


def _data(case, dtype):
    """Inputs on the GPU, the fp64 reference and the bounds, computed once per (case, dtype)."""
    key = (case, dtype)
    if key in _cache:
        return _cache[key]
    from pytorch_distributed_template_amd.ops import winattn as wa
    (Bw, nwin, heads, N), form, scale, _ = case
    gen = torch.Generator().manual_seed(Bw * 100 + N)
    C = heads * 32
    if form == "packed":
        qkv = torch.randn(Bw, N, 3, heads, 32, generator=gen).to(dtype).to(DEV)
        q, k, v = qkv.unbind(2)
    else:  # three tensors with padded token and head strides
        q, k, v = (torch.randn(Bw, N + 1, heads, 40, generator=gen).to(dtype).to(DEV)[:, :N, :, :32] for _ in range(3))
        qkv = None
    dy = torch.randn(Bw, N, C, generator=gen).to(dtype).to(DEV)
    bias = torch.randn(heads, N, N, generator=gen)
    if Bw == 3:
        bias[0, 5, 7] += 30.0
    bias = bias.to(DEV)
    region = None
    if nwin == 4:
        region = wa.region_labels(14, 14, 7, 3, 3, DEV)
        assert region.unique().numel() == 9
    elif nwin:
        region = torch.randint(0, 3, (nwin, N), generator=gen).to(torch.uint8).to(DEV)

    ref, bound = _bounds(q, k, v, dy, bias, region, scale, dtype)
    _cache[key] = dict(q=q, k=k, v=v, qkv=qkv, dy=dy, bias=bias, region=region, ref=ref, bound=bound)
    return _cache[key]


def _check(got, d, k, what):
    w = assert_within(got.reshape(d["ref"][k].shape), d["ref"][k], d["bound"][k], f"{what}: {k}", family="winattn_" + k)
    print(f"{what} {k}: max err / bound {w:.3e}")


def _nan(*shape, dtype):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def _run(d, case, dtype, max_blocks):
    """Forward and backward through the raw bindings into NaN-filled outputs and workspaces."""
    from pytorch_distributed_template_amd.ops import native, winattn as wa
    (Bw, nwin, heads, N), form, scale, _ = case
    mb = max_blocks or wa.MAX_BLOCKS
    y, stat = _nan(Bw, N, heads * 32, dtype=dtype), _nan(Bw, heads, N, 2, dtype=torch.float32)
    native.C.winattn_fwd(d["q"], d["k"], d["v"], d["bias"], d["region"], y, stat, scale, mb)
    blocks, slabs = wa.window_attention_plan(Bw, heads, N, mb)
    assert blocks * 4 == slabs * heads
    if form == "packed":  # one dense dqkv
        grads = _nan(Bw, N, 3, heads, 32, dtype=dtype).unbind(2)
    else:
        grads = [_nan(Bw, N + 1, heads, 40, dtype=dtype)[:, :N, :, :32] for _ in range(3)]
    ws = _nan(slabs, heads, N, N, dtype=torch.float32)
    got = native.C.winattn_bwd(d["dy"].view(Bw, N, heads, 32), d["q"], d["k"], d["v"], d["bias"], d["region"], stat,
                               *grads, ws, scale, mb)
    assert got == slabs
    return y, stat, grads, ws


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c[0])))
def test_forward(case, dtype):
    d = _data(case, dtype)
    y, stat, _, _ = _run(d, case, dtype, case[3])
    assert bool(torch.isfinite(stat).all())
    _check(y, d, "o", f"{case[0]} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c[0])))
def test_backward(case, dtype):
    from pytorch_distributed_template_amd.ops import winattn as wa
    d = _data(case, dtype)
    _, stat, (dq, dk, dv), ws = _run(d, case, dtype, case[3])
    what = f"{case[0]} {dtype}"
    for k, got in (("dq", dq), ("dk", dk), ("dv", dv)):
        _check(got, d, k, what)
    _check(ws.double().sum(0), d, "db", what + " slabs")
    db = wa.window_attention_bwd(d["dy"], d["q"], d["k"], d["v"], d["bias"], d["region"], stat, case[2],
                                 max_blocks=case[3])[3]
    _check(db, d, "db", what)


@pytest.mark.parametrize("dtype", DTYPES)
def test_bit_identical_and_plan_independent(dtype):
    """Twice through the same plan and once through other block counts (3 blocks: 4 slots; 150: 200 slots, the two-stage
    slab sum): every output equal bit for bit except dbias, whose summation order belongs to the plan."""
    from pytorch_distributed_template_amd.ops import winattn as wa
    case = CASES[4]
    (Bw, _, heads, N), _, scale, _ = case
    d = _data(case, dtype)
    a, b, c = _run(d, case, dtype, 6), _run(d, case, dtype, 6), _run(d, case, dtype, 3)
    assert [wa.window_attention_plan(Bw, heads, N, mb) for mb in (3, 150)] == [(3, 4), (150, 200)]
    for x, y, z in zip((a[0], a[1], *a[2]), (b[0], b[1], *b[2]), (c[0], c[1], *c[2])):
        assert torch.equal(x, y) and torch.equal(x, z)
    assert torch.equal(a[3], b[3])
    args = (d["dy"], d["q"], d["k"], d["v"], d["bias"], d["region"], a[1], scale)
    wide = [wa.window_attention_bwd(*args, max_blocks=150) for _ in range(2)]
    assert all(torch.equal(p, q) for p, q in zip(*wide)) and torch.equal(wide[0][0], a[2][0])
    _check(wide[0][3], d, "db", f"{case[0]} {dtype} 200 slabs")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", [CASES[1], CASES[4]], ids=["separate", "packed"])
def test_autograd_functions(case, dtype):
    """The two autograd functions as the modules call them: y and the gradients they hand to autograd, same bounds."""
    from pytorch_distributed_template_amd.ops import winattn as wa
    (Bw, _, heads, N), form, scale, _ = case
    d = _data(case, dtype)
    bias = d["bias"].clone().requires_grad_(True)
    if form == "packed":
        qkv = d["qkv"].reshape(Bw, N, 3 * heads * 32).clone().requires_grad_(True)
        y = wa._PackedFn.apply(qkv, bias, d["region"], heads, scale)
        y.backward(d["dy"])
        grads = qkv.grad.view(Bw, N, 3, heads, 32).unbind(2)
    else:
        leaves = [d[n].detach().requires_grad_(True) for n in "qkv"]
        y = wa._SeparateFn.apply(*leaves, bias, d["region"], scale)
        y.backward(d["dy"])
        grads = [t.grad for t in leaves]
    for k, got in zip(("o", "dq", "dk", "dv", "db"), (y, *grads, bias.grad)):
        _check(got, d, k, f"{form} function {dtype}")


def test_operand_strides():
    """A dimension of size 1 may carry any stride; an output view that overlaps itself is refused before the launch."""
    from pytorch_distributed_template_amd.ops import winattn as wa
    d = _data(CASES[0], torch.bfloat16)
    one = [d[n][:1] for n in "qkv"]
    odd = [torch.as_strided(t, t.shape, (3, t.stride(1), 5, 1), t.storage_offset()) for t in one]
    y, stat = wa.window_attention_fwd(*one, d["bias"], None, 1.0)
    assert torch.equal(wa.window_attention_fwd(*odd, d["bias"], None, 1.0)[0], y)
    out = [torch.empty(1, 1, 1, 32, dtype=torch.bfloat16, device=DEV).expand(1, 49, 1, 32) for _ in range(3)]
    with pytest.raises(RuntimeError, match="positive"):
        wa.window_attention_bwd(d["dy"][:1], *one, d["bias"], None, stat, 1.0, out=out)


def _counts():
    from pytorch_distributed_template_amd.ops import native
    c = native.C.dispatch_counts()
    return [c.get(k, 0) for k in ("winattn_fwd", "winattn_bwd")]


@pytest.mark.parametrize("kind", ["swin", "swin_v2", "maxvit"])
def test_converted_module_trains(kind):
    """A shifted Swin block (14 x 14 tokens, window 7), a shifted Swin V2 block (16 x 16, window 8: N = 64, separate
    q / k) and a MaxViT layer, B = 2, dim 96, 3 heads, one training step under bf16 autocast.  The attention the
    module ran is read off the autograd node of the y it hands to its projection and held to the derived bounds,
    forward and backward.  Its inputs are checked where that is exact: scale, region table, the fp32 bias, and for V2
    the row norms of q (the clamped logit scale) and k (1), each element rounded to bf16 at most twice: 2 * 2**-9.
    The block output and parameter gradients pass through bf16 Linears: no bound was derived, none is asserted."""
    from pytorch_distributed_template_amd.models import modern
    from pytorch_distributed_template_amd.ops import winattn as wa
    torch.manual_seed(3)
    if kind == "maxvit":
        block = modern.PartitionAttentionLayer(96, 32, 7, "window", 14, 4, 0.0, 0.0, 0.0).to(DEV)
        attn, x, N = block.attn_layer[1], torch.randn(2, 96, 14, 14, device=DEV), 49
        with torch.no_grad():
            attn.relative_position_bias_table.normal_()  # a bias that matters
    else:
        side, win = (14, 7) if kind == "swin" else (16, 8)
        block = modern.SwinTransformerBlock(96, 3, win, win // 2, 0.0, v2=kind == "swin_v2").to(DEV)
        attn, x, N = block.attn, torch.randn(2, side, side, 96, device=DEV), win * win
        with torch.no_grad():
            (attn.cpb_mlp[2].weight if attn.v2 else attn.relative_position_bias_table).normal_()
    assert wa.convert_window_attention(block) == 1
    attn, seen = (block.attn_layer[1] if kind == "maxvit" else block.attn), {}

    def grab(_, inputs):  # the projection's input is the attention's y: its autograd node holds the rest
        node = inputs[0].grad_fn
        seen.update(y=inputs[0].detach(), saved=node.saved_tensors, region=node.region, scale=node.scale)
        node.register_hook(lambda gin, gout: seen.update(gin=gin, dy=gout[0]))

    (attn.merge if kind == "maxvit" else attn.proj).register_forward_pre_hook(grab)
    before = _counts()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = block.train()(x)
        bias = (attn.get_relative_positional_bias() if kind == "maxvit" else attn._bias())[0].float()
    out.backward(torch.randn_like(out))
    assert [a - b for a, b in zip(_counts(), before)] == [1, 1]

    *qkv, b, _ = seen["saved"]
    q, k, v = qkv if len(qkv) == 3 else qkv[0].view(8, N, 3, 3, 32).unbind(2)
    assert q.shape == (8, N, 3, 32) and q.dtype == torch.bfloat16 and torch.equal(b, bias)
    assert seen["scale"] == {"swin": 32 ** -0.5, "swin_v2": 1.0, "maxvit": 96 ** -0.5}[kind]
    if kind == "maxvit":
        assert seen["region"] is None
    else:
        assert torch.equal(seen["region"], wa.region_labels(side, side, win, win // 2, win // 2, DEV))
    if kind == "swin_v2":
        want = torch.clamp(attn.logit_scale, max=4.605170185988092).exp().view(1, 1, 3)
        assert bool(((q.double().norm(dim=-1) / want - 1).abs() <= 2.0 ** -8).all())
        assert bool(((k.double().norm(dim=-1) - 1).abs() <= 2.0 ** -8).all())
    ref, bound = _bounds(q, k, v, seen["dy"], b, seen["region"], seen["scale"], torch.bfloat16)
    gin = seen["gin"]
    grads = gin[:3] if len(qkv) == 3 else gin[0].view(8, N, 3, 3, 32).unbind(2)
    for name, got in zip(("o", "dq", "dk", "dv", "db"), (seen["y"], *grads, gin[3] if len(qkv) == 3 else gin[1])):
        w = assert_within(got.reshape(ref[name].shape), ref[name], bound[name], f"{kind} module: {name}",
                          family="winattn_module_" + name)
        print(f"{kind} module {name}: max err / bound {w:.3e}")
