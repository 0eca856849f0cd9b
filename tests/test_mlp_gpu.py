"""GELU-MLP HIP kernels (csrc/kernels/mlp.hip) and the converted Sequential on an MI355X.

References are fp64 on the CPU from the very 16-bit ``z0``, ``dy``, ``w2`` and fp32 ``b1``, ``b2`` the kernels read, with
no intermediate rounding: v = z0 + b1, h = gelu(v) = v (1 + erf(v / sqrt 2)) / 2, gelu'(v) = Phi(v) + v phi(v).  Bounds
are per element, from ``tests/_numerics.py`` (u = 2^-24), with eps(v) = K * u * max(1, |v|) for the kernels' fp32 GELU
(K_G) and derivative (K_DG):

    y   : conv_bound(n = Hd) + sum_j |w2[c][j]| (half_ulp16(h_j) + eps_g(v_j))       h is rounded into the MFMA operand
    dz  : half_ulp16(ref) + (Co + 4) 2u mag |gelu'(v)| + |dy w2| eps_g'(v)
    db1 : the fp64 column sum of the dz the kernel RETURNED, assert_sum with the launch's chain
    dw2 : (chain + 4) u mag (assert_sum's formula, the plan's chain) + sum_m |dy| (half_ulp16(h) + eps_g)

K_G and K_DG were measured on the CPU against torch, never against the kernels: the worst error of fp32 ``F.gelu`` (and
of the analytic derivative evaluated with fp32 torch ops) against fp64 over 2^18 points per unit of v in [-12, 12], in
units of u * max(1, |v|), is 6.38 (the cancellation in 1 + erf for v < 0) and 2.30; both are doubled, since another erf
of equal quality may err the other way.  Largest error / bound ratios: profiles/mlp_mi355x.md.
"""
import copy
import math

import pytest
import torch

from _numerics import U, assert_sum, assert_within, conv_bound, half_ulp16

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
K_G = 12.8   # 2 * 6.38 (measured 6.3809), rounded up
K_DG = 4.6   # 2 * 2.30 (measured 2.2972)
WIDTHS = [(8, 8, 8), (24, 40, 24), (96, 384, 96), (264, 1056, 264)]  # (C, Hd, Co); 264: a second column block
# M: a lone row, tails past one and several row tiles; the contract's corner at M = 130 only
CASES = [(M,) + w for w in WIDTHS for M in (1, 130, 517)] + [(130, 512, 2048, 512)]
_cases = lambda f: pytest.mark.parametrize("dtype", DTYPES)(
    pytest.mark.parametrize("case", CASES, ids=["x".join(map(str, c)) for c in CASES])(f))
_cache = {}


def _gelu64(v):
    return 0.5 * v * (1 + torch.erf(v / math.sqrt(2)))


def _dgelu64(v):
    return 0.5 * (1 + torch.erf(v / math.sqrt(2))) + v * torch.exp(-0.5 * v * v) / math.sqrt(2 * math.pi)


def _data(case, dtype):
    """Inputs on the GPU (z0 from the existing pwconv_fwd) and the fp64 references, once per (case, dtype)."""
    if (case, dtype) not in _cache:
        from pytorch_distributed_template_amd.ops import pointwise
        M, C, Hd, Co = case
        gen = torch.Generator().manual_seed(M * 1000 + Hd)
        rn = lambda *shape: torch.randn(*shape, generator=gen)
        x, w1 = rn(M, C).to(dtype).to(DEV), (rn(Hd, C) * 1.5 * C ** -0.5).to(dtype).to(DEV)
        b1, w2, b2, dy = rn(Hd) * 0.5, (rn(Co, Hd) * Hd ** -0.5).to(dtype), rn(Co) * 0.5, rn(M, Co).to(dtype)
        z0 = pointwise.pwconv_fwd(x, w1)
        v = z0.cpu().double() + b1.double()
        W, D = w2.double(), dy.double()
        h, dg, eps = _gelu64(v), _dgelu64(v), U * v.abs().clamp_min(1)
        e_h = half_ulp16(h, dtype) + K_G * eps  # the error of the rounded h operand
        y = h @ W.T + b2.double()
        t = D @ W
        ref = dict(y=y, dz=t * dg, dw2=D.T @ h)
        bound = dict(y=conv_bound(y, h.abs() @ W.abs().T + b2.double().abs(), Hd, dtype) + e_h @ W.abs().T,
                     dz=half_ulp16(ref["dz"], dtype) + (Co + 4) * 2 * U * (D.abs() @ W.abs()) * dg.abs()
                     + t.abs() * K_DG * eps,
                     dw2_carried=D.abs().T @ e_h, dw2_mag=D.abs().T @ h.abs())
        _cache[case, dtype] = dict(z0=z0, x=x, w1=w1, ref=ref, bound=bound,
                                   **{k: t.to(DEV) for k, t in dict(b1=b1, w2=w2, b2=b2, dy=dy).items()})
    return _cache[case, dtype]


def _count(name):
    from pytorch_distributed_template_amd.ops import native
    return native.C.dispatch_counts().get(name, 0)


@_cases
def test_kernels(case, dtype):
    from pytorch_distributed_template_amd.ops import mlp
    M, C, Hd, Co = case
    d = _data(case, dtype)
    ref, bound = d["ref"], d["bound"]
    assert mlp.mlp_fits(M, C, Hd, Co)
    before = [_count(k) for k in ("mlp_fc2_fwd", "mlp_fc2_dgrad", "mlp_fc2_wgrad")]

    y = mlp.mlp_fc2_fwd(d["z0"], d["b1"], d["w2"], d["b2"])
    assert y.dtype == dtype and y.shape == (M, Co)
    w = assert_within(y.cpu(), ref["y"], bound["y"], f"{case} y", Co, "mlp_fwd", ref["y"].shape)
    print(f"{case} y: max err / bound {w:.3e}")

    # the default launch, and one capped to 2 blocks per slice: every block walks several tiles
    for cap in (0, 2 * ((Hd + 127) // 128)) if M == 517 else (0,):
        dz, db1, (rows, chain) = mlp.mlp_fc2_dgrad(d["dy"], d["w2"], d["z0"], d["b1"], cap)
        assert dz.dtype == dtype and db1.dtype == torch.float32 and 1 <= rows <= (M + 127) // 128
        w = assert_within(dz.cpu(), ref["dz"], bound["dz"], f"{case} dz cap={cap}", Hd, "mlp_dgrad", ref["dz"].shape)
        dz64 = dz.cpu().double()
        ws = assert_sum(db1.cpu(), dz64.sum(0), dz64.abs().sum(0), chain, f"{case} db1 cap={cap}", Hd, "mlp_db1")
        print(f"{case} cap={cap} dz: {w:.3e}  db1 (chain {chain}): {ws:.3e}")

    # the default plan, and a small target: several splits with a ragged last one
    for target in (mlp.WGRAD_TARGET_BLOCKS, 3 * ((Hd + 63) // 64) * ((Co + 63) // 64)) if M == 517 else (mlp.WGRAD_TARGET_BLOCKS,):
        splits, rps, _, _, chain = mlp.mlp_fc2_wgrad_plan(M, Hd, Co, target)
        if target != mlp.WGRAD_TARGET_BLOCKS:
            assert splits == 3 and 0 < M - 2 * rps < rps
        dw2 = mlp.mlp_fc2_wgrad(d["z0"], d["b1"], d["dy"], target)
        assert dw2.dtype == torch.float32 and dw2.shape == (Co, Hd)
        w = assert_within(dw2.cpu(), ref["dw2"], (chain + 4) * U * bound["dw2_mag"] + bound["dw2_carried"],
                          f"{case} dw2 target={target}", Hd, "mlp_wgrad", ref["dw2"].shape)
        print(f"{case} target={target} dw2 (splits {splits}, chain {chain}): {w:.3e}")
    assert [_count(k) for k in ("mlp_fc2_fwd", "mlp_fc2_dgrad", "mlp_fc2_wgrad")] == \
        [b + n for b, n in zip(before, (1, 2, 2) if M == 517 else (1, 1, 1))]


@pytest.mark.parametrize("dtype", DTYPES)
def test_cnblock_against_fp64(dtype):
    """One ConvNeXt block, forward and backward under autocast, converted against stock: the output, dx and every
    parameter gradient against the fp64 block, the converted arm's worst error within twice the stock arm's."""
    from pytorch_distributed_template_amd.models.modern import CNBlock
    from pytorch_distributed_template_amd.ops import mlp
    torch.manual_seed(3)
    stock = torch.nn.Sequential(CNBlock(24, 1.0, 0.0))
    with torch.no_grad():
        for p in stock.parameters():
            if p.dim() == 1:
                p.add_(torch.randn_like(p) * 0.2)  # biases and LayerNorm off their initial 0 / 1
    x, gy = torch.randn(2, 24, 9, 9), torch.randn(2, 24, 9, 9)
    ref_m = copy.deepcopy(stock).double()
    native_m = copy.deepcopy(stock).to(DEV)
    stock = stock.to(DEV)
    assert mlp.convert_mlp(native_m) == 1 and type(native_m[0].block) is mlp.NativeMLPSequential

    def run(m, x, gy, autocast):
        x = x.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=dtype, enabled=autocast):
            y = m(x)
        y.backward(gy.to(y.dtype))
        return [y.detach(), x.grad] + [p.grad for p in m.parameters()]

    ref = run(ref_m, x.double(), gy.double(), False)
    before = _count("mlp_fc2_fwd"), _count("mlp_fc2_dgrad"), _count("mlp_fc2_wgrad")
    got = run(native_m, x.to(DEV), gy.to(DEV), True)
    assert (_count("mlp_fc2_fwd"), _count("mlp_fc2_dgrad"), _count("mlp_fc2_wgrad")) == tuple(b + 1 for b in before)
    base = run(stock, x.to(DEV), gy.to(DEV), True)
    names = ["y", "dx"] + [k for k, _ in ref_m.named_parameters()]
    assert len(ref) == len(got) == len(base) == len(names) == 11
    for k, r, g, b in zip(names, ref, got, base):
        assert g.dtype == b.dtype and g.shape == r.shape
        e_native, e_stock = (g.cpu().double() - r).abs().max().item(), (b.cpu().double() - r).abs().max().item()
        print(f"{k}: native {e_native:.3e} stock {e_stock:.3e}")
        assert e_native <= 2 * e_stock, f"{k}: native error {e_native:.3e} > 2 x stock error {e_stock:.3e}"
    # without autocast (the torch engine's validation) the children run as nn.Sequential runs them
    assert torch.equal(native_m(x.to(DEV)), stock(x.to(DEV)))
    assert _count("mlp_fc2_fwd") == before[0] + 1
