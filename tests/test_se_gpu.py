"""Squeeze-and-excitation HIP kernels (csrc/kernels/se.hip) and the converted modules on an MI355X.

References are the plain fp64 formulas on the CPU from the rounded inputs, with the sums over all of N and HW in fp64.
Bounds are per element, counted from the kernels' fp32 roundings (t = 2^-24), not tuned; a sum of n fp32 terms in any
order errs by at most n * t * sum|term|.  With A = |W1|, B = |W2| and, for the exp2 and reciprocal units (1 ulp = 2t each,
exp2 flushing subnormal results) behind sigmoid(v) = 1 / (1 + exp2(-v * log2 e)),

    unit(v) = sigmoid(v) * (2|v| + 6) * t + 2^-126       -v * log2 e: two roundings, worth |v| * 2t in the result;
                                                         exp2 2t, the add t, the reciprocal 2t, one spare
forward:
    e_z = (HW + 2) * t * mean|x|                         the HW-term sum, then the product with the rounded 1 / HW
    e_u = A e_z + (C + 2) * t * (A |z| + |b1|)           the C-term dot product and the bias
    e_h = e_u (relu)  |  1.1 e_u + |u| unit(u) + t |h|   silu's slope is below 1.1
    e_v = B e_h + (S + 2) * t * (B |h| + |b2|)
    e_s = e_v / 4 + unit(v) (sigmoid: slope <= 1/4)  |  e_v / 6 + 2t (|v| / 6 + 1/2) (hardsigmoid: slope 1/6)
    |y - ref| <= u |ref| + |x| e_s + t |ref| + sub
backward, ds = sum_hw dy x, gate' = s (1 - s) or 1/6 inside (-3, 3), act' = [u > 0] or sig(u) (1 + u (1 - sig(u))):
    e_ds = (HW + 2) * t * sum|dy x|
    e_g' = e_s + 3t gate' (sigmoid)  |  t / 6 (hardsigmoid, the region is the reference's: see the margins)
    e_dv = (gate' + e_g') e_ds + |ds| e_g' + t |dv|
    e_dh = B^T e_dv + (C + 2) * t * B^T |dv|
    e_a' = 0 (relu)  |  e_u / 2 + (1 + |u|) (unit(u) + 6t) (silu: |silu''| <= 1/2, four more operations)
    e_du = (|act'| + e_a') e_dh + |dh| e_a' + t |du|
    e_g  = (A^T e_du + (S + 3) * t * A^T |du|) / HW
    |dx - ref|  <= u |ref| + |dy| e_s + e_g + 2t (|dy s| + |g|) + sub
    |dW2 - ref| <= sum_n (e_dv (|h| + e_h) + |dv| e_h) + (N + 2) * t * sum_n |dv h|       h recomputed from u: e_h again
    |db2 - ref| <= sum_n e_dv + N t sum_n |dv|
    |dW1 - ref| <= sum_n (e_du (|z| + e_z) + |du| e_z) + (N + 2) * t * sum_n |du z|
    |db1 - ref| <= sum_n e_du + N t sum_n |du|
with u = 2^-8 (bf16) or 2^-11 (fp16) for the one rounding of y and dx and sub one subnormal step.  ReLU's zero and
hardsigmoid's kinks are discontinuities of the derivative: ``_data`` asserts that every reference u (relu) is further
from 0 than e_u and every v (hardsigmoid) further from +-3 than e_v + 16t (the gate's own rounding), so no case is
skipped at run time.  The bounds are worst cases over summation orders: a correct kernel passes by construction, and a
ratio near 1 means the count is wrong (largest ratios: profiles/se_mi355x.md).
"""
import pytest
import torch
import torch.nn as nn

from _numerics import assert_within

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
U16 = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
T = 2.0 ** -24
# (N, HW, C, S, act, gate)
CASES = [
    (1, 1, 8, 1, "relu", "sigmoid"),            # one row, one vector, S = 1
    (3, 49, 40, 6, "silu", "sigmoid"),          # masked channel vectors (5 groups, 51 row lanes), ragged rows, odd S
    (2, 196, 96, 4, "silu", "sigmoid"),         # two chunks per image
    (5, 49, 1152, 48, "silu", "sigmoid"),       # wide C on a small map: one row lane, 144 of 256 threads
    (2, 3136, 32, 8, "silu", "sigmoid"),        # seven HW chunks per image; again with max_blocks = 1
    (4, 25, 72, 24, "relu", "hardsigmoid"),
    (1, 7, 4096, 512, "relu", "sigmoid"),       # the contract's corner: two column chunks, two images per gate block
    (9, 4, 16, 8, "relu", "hardsigmoid"),       # N not a multiple of the gate kernels' image group
    (3, 25, 104, 26, "relu", "sigmoid"),        # the _RegNetSE of the module test
]
KERNELS = ("se_pool", "se_gate", "se_scale", "se_bwd_reduce", "se_gate_bwd", "se_wgrad", "se_bwd_apply")
_cases = lambda f: pytest.mark.parametrize("dtype", DTYPES)(
    pytest.mark.parametrize("case", CASES, ids=["x".join(map(str, c)) for c in CASES])(f))
_cache = {}


def _ref(x, dy, w1, b1, w2, b2, act, gate):
    """fp64 reference and the bounds of the module docstring; x, dy: [N, HW, C]; w1 [S, C], w2 [C, S]."""
    N, HW, C = x.shape
    S = w1.shape[0]
    x, dy, w1, b1, w2, b2 = (t.detach().double().cpu() for t in (x, dy, w1, b1, w2, b2))
    A, B, sig = w1.abs(), w2.abs(), torch.sigmoid
    unit = lambda v: sig(v) * (2 * v.abs() + 6) * T + 2.0 ** -126
    z = x.mean(1)
    u = z @ w1.T + b1
    h = u.clamp_min(0) if act == "relu" else u * sig(u)
    v = h @ w2.T + b2
    s = sig(v) if gate == "sigmoid" else (v / 6 + 0.5).clamp(0, 1)
    ds = (dy * x).sum(1)
    gp = s * (1 - s) if gate == "sigmoid" else ((v > -3) & (v < 3)).double() / 6
    dv = ds * gp
    dh = dv @ w2
    ap = (u > 0).double() if act == "relu" else sig(u) * (1 + u * (1 - sig(u)))
    du = dh * ap
    g = du @ w1 / HW
    ref = dict(z=z, u=u, s=s, y=x * s[:, None], dx=dy * s[:, None] + g[:, None], dw2=dv.T @ h, db2=dv.sum(0),
               dw1=du.T @ z, db1=du.sum(0))
    e_z = (HW + 2) * T * x.abs().mean(1)
    e_u = e_z @ A.T + (C + 2) * T * (z.abs() @ A.T + b1.abs())
    e_h = e_u if act == "relu" else 1.1 * e_u + u.abs() * unit(u) + T * h.abs()
    e_v = e_h @ B.T + (S + 2) * T * (h.abs() @ B.T + b2.abs())
    e_s = e_v / 4 + unit(v) if gate == "sigmoid" else e_v / 6 + 2 * T * (v.abs() / 6 + 0.5)
    if act == "relu":
        assert bool((u.abs() > e_u).all()), "a reference u within its bound of ReLU's zero: change the seed"
    if gate == "hardsigmoid":
        assert bool(((v.abs() - 3).abs() > e_v + 16 * T).all()), "a reference v at a hardsigmoid kink: change the seed"
    e_ds = (HW + 2) * T * (dy * x).abs().sum(1)
    e_gp = e_s + 3 * T * gp if gate == "sigmoid" else torch.full_like(gp, T / 6)
    e_dv = (gp + e_gp) * e_ds + ds.abs() * e_gp + T * dv.abs()
    e_dh = e_dv @ B + (C + 2) * T * (dv.abs() @ B)
    e_ap = torch.zeros_like(u) if act == "relu" else e_u / 2 + (1 + u.abs()) * (unit(u) + 6 * T)
    e_du = (ap.abs() + e_ap) * e_dh + dh.abs() * e_ap + T * du.abs()
    e_g = (e_du @ A + (S + 3) * T * (du.abs() @ A)) / HW
    bound = dict(
        z=e_z, u=e_u, s=e_s, y=x.abs() * e_s[:, None] + T * ref["y"].abs(),
        dx=dy.abs() * e_s[:, None] + e_g[:, None] + 2 * T * ((dy * s[:, None]).abs() + g.abs()[:, None]),
        dw2=e_dv.T @ (h.abs() + e_h) + dv.abs().T @ e_h + (N + 2) * T * (dv.abs().T @ h.abs()),
        db2=e_dv.sum(0) + N * T * dv.abs().sum(0),
        dw1=e_du.T @ (z.abs() + e_z) + du.abs().T @ e_z + (N + 2) * T * (du.abs().T @ z.abs()),
        db1=e_du.sum(0) + N * T * du.abs().sum(0))
    return ref, bound


def _data(case, dtype):
    """Inputs on the GPU (x, dy: NHWC [N, HW, 1, C]), the fp64 reference and the bounds, once per (case, dtype)."""
    if (case, dtype) not in _cache:
        N, HW, C, S, act, gate = case
        gen = torch.Generator().manual_seed(N * 1000 + C)
        rn = lambda *shape: torch.randn(*shape, generator=gen)
        x, dy = rn(N, HW, 1, C).to(dtype), rn(N, HW, 1, C).to(dtype)
        sign = lambda n: torch.where(torch.arange(n) % 2 == 0, 0.5, -0.5)
        w1, b1, w2, b2 = rn(S, C, 1, 1) * C ** -0.5 / 4, sign(S), rn(C, S, 1, 1) * S ** -0.5, sign(C)
        if gate == "hardsigmoid":
            b2[::4] *= 8  # +-4: both saturated branches
        ref, bound = _ref(x.view(N, HW, C), dy.view(N, HW, C), w1.view(S, C), b1, w2.view(C, S), b2, act, gate)
        _cache[case, dtype] = dict(x=x.to(DEV), dy=dy.to(DEV), p=[t.to(DEV) for t in (w1, b1, w2, b2)], ref=ref,
                                   bound=bound)
    return _cache[case, dtype]


def _check(got, d, k, what):
    ref, bound = d["ref"][k], d["bound"][k]
    if got.dtype in U16:  # the one rounding of a stored activation
        fi = torch.finfo(got.dtype)
        bound = bound + U16[got.dtype] * ref.abs() + fi.smallest_normal * fi.eps
    w = assert_within(got.detach().cpu().reshape(ref.shape), ref, bound, f"{what}: {k}", family="se_" + k)
    print(f"{what} {k}: max err / bound {w:.3e}")


def _counts():
    from pytorch_distributed_template_amd.ops import native
    c = native.C.dispatch_counts()
    return [c.get(k, 0) for k in KERNELS]


def _delta(before):
    return [a - b for a, b in zip(_counts(), before)]


@_cases
def test_fwd_bwd(case, dtype):
    from pytorch_distributed_template_amd.ops import se
    N, HW, C, S, act, gate = case
    d = _data(case, dtype)
    caps = (None, 1) if case[:3] == (2, 3136, 32) else (None,)
    if len(caps) == 2:
        assert se.se_plan(N, HW, C)[0] == 7 and se.se_plan(N, HW, C, 1) == (1, HW)
    for mb in caps:
        what = f"{case} cap={mb}"
        before = _counts()
        y, z, u, s = se.se_fwd(d["x"], *d["p"], act, gate, mb)
        assert _delta(before) == [1, 1, 1, 0, 0, 0, 0] and y.dtype == dtype and z.dtype == u.dtype == s.dtype == torch.float32
        for k, got in (("y", y), ("z", z), ("u", u), ("s", s)):
            _check(got, d, k, what)
        w1, _, w2, _ = d["p"]
        out = se.se_bwd(d["dy"], d["x"], w1, w2, z, u, s, act, gate, max_blocks=mb)
        assert _delta(before) == [1] * 7 and out[0].dtype == dtype and all(t.dtype == torch.float32 for t in out[1:])
        for k, got in zip(("dx", "dw1", "db1", "dw2", "db2"), out):
            _check(got, d, k, what)


@pytest.mark.parametrize("dtype", DTYPES)
def test_repeatable_and_skipped_outputs(dtype):
    """Twice the same bits; with requires_grad on x alone, then on the parameters alone, the skipped gradients are None,
    their kernels do not run and the others keep their bits."""
    from pytorch_distributed_template_amd.ops import se
    case = CASES[1]
    d = _data(case, dtype)
    nchw = lambda t: t.permute(0, 3, 1, 2)

    def run(on_x, on_p):
        x = nchw(d["x"]).detach().requires_grad_(on_x)
        p = [t.detach().requires_grad_(on_p) for t in d["p"]]
        before = _counts()
        y = se._SEFn.apply(x, *p, case[4], case[5])
        y.backward(nchw(d["dy"]))
        return [y.detach(), x.grad] + [t.grad for t in p], _delta(before)

    full, n_full = run(True, True)
    again, _ = run(True, True)
    assert n_full == [1] * 7 and all(torch.equal(a, b) for a, b in zip(full, again))
    only_x, n_x = run(True, False)
    assert n_x == [1, 1, 1, 1, 1, 0, 1] and all(g is None for g in only_x[2:]) and torch.equal(only_x[1], full[1])
    only_p, n_p = run(False, True)
    assert n_p == [1, 1, 1, 1, 1, 1, 0] and only_p[1] is None
    assert all(torch.equal(a, b) for a, b in zip(only_p[2:], full[2:]))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", [CASES[2], CASES[8]], ids=["SqueezeExcitation", "RegNetSE"])
def test_module_path(case, dtype):
    from pytorch_distributed_template_amd.models import efficient, modern
    from pytorch_distributed_template_amd.ops import se
    N, HW, C, S, act, gate = case
    d = _data(case, dtype)
    stock = efficient.SqueezeExcitation(C, S, nn.SiLU, nn.Sigmoid) if act == "silu" else modern._RegNetSE(C, S)
    stock = stock.to(DEV)
    with torch.no_grad():
        for p, v in zip((stock.fc1.weight, stock.fc1.bias, stock.fc2.weight, stock.fc2.bias), d["p"]):
            p.copy_(v)
    model = nn.Sequential(stock)
    assert se.convert_se(model) == 1
    m = model[0]
    x = d["x"].permute(0, 3, 1, 2).detach().requires_grad_(True)  # NCHW view of NHWC storage: dense channels_last
    before = _counts()
    y = m(x)
    assert _delta(before) == [1, 1, 1, 0, 0, 0, 0] and y.dtype == dtype and y.permute(0, 2, 3, 1).is_contiguous()
    y.backward(d["dy"].permute(0, 3, 1, 2))
    assert _delta(before) == [1] * 7
    what = f"module {case}"
    _check(y.permute(0, 2, 3, 1), d, "y", what)
    _check(x.grad.permute(0, 2, 3, 1), d, "dx", what)
    for k, p in (("dw1", m.fc1.weight), ("db1", m.fc1.bias), ("dw2", m.fc2.weight), ("db2", m.fc2.bias)):
        assert p.grad.dtype == torch.float32 and p.grad.shape == p.shape
        _check(p.grad, d, k, what)
    before = _counts()  # fp32 (the torch engine's validation) and NCHW-contiguous inputs take the parent's forward
    assert torch.equal(m(x.detach().float()), stock(x.detach().float()))
    with torch.autocast("cuda", dtype=dtype):
        assert torch.equal(m(x.detach().contiguous()), stock(x.detach().contiguous()))
    assert _delta(before) == [0] * 7
