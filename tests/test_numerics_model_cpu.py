"""The error model of tests/_numerics.py can pass and can fail (CPU only).

* A plain torch-fp32 evaluation of every formula, rounded with ``.to(dtype)``, stays inside its bound: the bounds are
  reachable by a correct implementation (observed here: bn_apply 0.99-0.9999 of the bound -- the half-ulp term is
  tight by construction --, the reduce chain ~0.006, SGD over 3 steps ~0.14, the finalize outputs 0.24-0.61).
* Each assertion rejects one element off by one 16-bit ulp, one row missing from a 3000-row sum, and coefficients
  shifted by one channel.
* The backward formula the GPU tests use as their reference (dy = A*dz + B*y + Cc, dgamma = sum dz*xhat,
  dbeta = sum dz) equals torch.autograd of F.batch_norm in fp64 to 1e-10.
"""
import math

import pytest
import torch
import torch.nn.functional as F

import _numerics as nm

DTYPES = [torch.bfloat16, torch.float16]


def _apply_case(C, dtype, rows=257, seed=0):
    g = torch.Generator().manual_seed(seed + C)
    y = (torch.randn(rows, C, generator=g) * 2).to(dtype)
    res = torch.randn(rows, C, generator=g).to(dtype)
    coef = torch.cat([torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3,
                      torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5])
    rcoef = torch.cat([torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3])
    # one channel at 1e-6 scale: fp16 outputs in the subnormal range
    coef[1] *= 1e-6
    coef[C + 1] *= 1e-6
    rcoef[1] *= 1e-6
    rcoef[C + 1] *= 1e-6
    return y, res, coef, rcoef


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [8, 192, 2048])
@pytest.mark.parametrize("resmode,relu", [(0, True), (1, False), (2, True), (2, False)])
def test_fp32_emulation_of_bn_apply_stays_within_the_bound(C, dtype, resmode, relu):
    y, res, coef, rcoef = _apply_case(C, dtype)
    if resmode == 1:  # the identity residual of the small channel must be small too to reach the subnormals
        res[:, 1] = (res[:, 1].float() * 1e-6).to(dtype)
    out = nm.bn_apply_emul(y, coef, res, rcoef, C, resmode, relu).to(dtype)
    _, ref, mag = nm.bn_apply_ref(y, coef, res, rcoef, C, resmode, relu)
    worst = nm.assert_rounded(out, ref, mag, dtype, name="bn_apply emulation", C=C)
    assert 0.5 < worst <= 1.0  # the half-ulp term is tight: a correct rounding comes close to it
    if dtype == torch.float16 and resmode != 1:
        assert bool((out[:, 1].float().abs() < 2.0 ** -14).any())  # subnormal outputs were exercised


@pytest.mark.parametrize("dtype", DTYPES)
def test_fp32_emulation_of_bwd_apply_stays_within_the_bound(dtype):
    C = 192
    y, g, _, _ = _apply_case(C, dtype, seed=3)
    b = torch.randn(3 * C, generator=torch.Generator().manual_seed(1))
    dz64 = g.to(torch.float64)
    out = (b[:C] * g.float() + b[C:2 * C] * y.float() + b[2 * C:]).to(dtype)
    ref, mag = nm.bn_bwd_apply_ref(dz64, y, b, C)
    nm.assert_rounded(out, ref, mag, dtype, name="bn_bwd_apply emulation", C=C)


def _reduce_case(rows, C, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    dz = torch.randn(rows, C, generator=g).to(dtype)
    y = (torch.randn(rows, C, generator=g) * 1.5 + 0.3).to(dtype)
    mean, invstd = torch.randn(C, generator=g) * 0.1 + 0.3, torch.rand(C, generator=g) + 0.5
    return dz, y, mean, invstd


def _reduce_ref(dz, y, mean, invstd):
    dz64 = dz.to(torch.float64)
    xh = (y.to(torch.float64) - mean.to(torch.float64)) * invstd.to(torch.float64)
    return dz64.sum(0), (dz64 * xh).sum(0), dz64.abs().sum(0), (dz64 * xh).abs().sum(0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_fp32_emulation_of_the_reduce_chain_stays_within_the_bound(dtype):
    rows, C, blocks, rpi = 3000, 128, 12, 16
    dz, y, mean, invstd = _reduce_case(rows, C, dtype)
    s0, s1, m0, m1 = _reduce_ref(dz, y, mean, invstd)
    # the kernel's structure: row r goes to chain (r // rpi % blocks, r % rpi); fp32 chains, then an fp32 sum over the
    # rpi lanes of a block, then fp64 over blocks
    xh = (y.float() - mean) * invstd
    n_chain = math.ceil(rows / (blocks * rpi)) + rpi
    pad = (-rows) % (blocks * rpi)
    for terms, ref, mag in ((dz.float(), s0, m0), (dz.float() * xh, s1, m1)):
        t = torch.cat([terms, torch.zeros(pad, C)]).view(-1, blocks, rpi, C)
        chain = torch.zeros(blocks, rpi, C)
        for i in range(t.shape[0]):
            chain = chain + t[i]
        blk = torch.zeros(blocks, C)
        for r in range(rpi):
            blk = blk + chain[:, r]
        worst = nm.assert_sum(blk.double().sum(0), ref, mag, n_chain, name="reduce emulation", C=C)
        assert worst < 0.5  # rounding errors average out: far below the worst-case chain bound


def test_fp32_emulation_of_sgd_stays_within_the_bound():
    g = torch.Generator().manual_seed(2)
    n = 10007
    p, gr = torch.randn(n, generator=g), torch.randn(n, generator=g)
    wdm = (torch.rand(n, generator=g) < 0.5).float()
    lr, mom, wd, gs = 0.1, 0.9, 1e-4, 0.125
    rp, rb, bound = nm.sgd_ref(p, gr, torch.zeros(n), wdm, lr, mom, wd, gs, 3)
    pe, be = p.clone(), torch.zeros(n)
    for step in range(3):
        d = gr * gs + wd * pe * wdm
        be = d if step == 0 else mom * be + d
        pe = pe - lr * be
    worst = nm.assert_within(pe, rp, bound, "sgd emulation: p")
    nm.assert_within(be, rb, bound / 0.1, "sgd emulation: buf")
    assert worst < 0.5


@pytest.mark.parametrize("C", [8, 200, 2048])
def test_fp32_emulation_of_finalize_stays_within_the_bounds(C):
    g = torch.Generator().manual_seed(C)
    rows = 3001
    x = (torch.randn(rows, C, generator=g) * (torch.rand(C, generator=g) * 3) + (torch.rand(C, generator=g) * 10 - 5))
    x = x.to(torch.bfloat16).double()
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    rm, rv = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    eps, mom = 1e-5, 0.1
    ref = nm.bn_finalize_ref(x.sum(0), (x * x).sum(0), float(rows), gamma, beta, eps, mom, rm, rv)
    # what the kernel does: fp64 statistics, rounded to fp32, then fp32 coefficient arithmetic
    mean32, invstd32 = ref["mean"].float(), ref["invstd"].float()
    sc = gamma * invstd32
    coef = torch.cat([sc, beta - mean32 * sc, mean32, invstd32])
    unb = (ref["var"] * rows / (rows - 1)).float()
    rm2 = (1.0 - torch.tensor(mom)) * rm + torch.tensor(mom) * mean32
    rv2 = (1.0 - torch.tensor(mom)) * rv + torch.tensor(mom) * unb
    worst = nm.check_finalize(coef, rm2, rv2, ref, C, "finalize emulation")
    assert worst <= 1.0
    # and the fp64 reference itself is torch's batch norm statistics
    assert torch.allclose(ref["mean"], x.mean(0), rtol=1e-12, atol=1e-12)
    assert torch.allclose(ref["var"], x.var(0, unbiased=False), rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("dtype", DTYPES)
def test_assert_rounded_rejects_one_element_off_by_one_ulp(dtype):
    C = 64
    y, res, coef, rcoef = _apply_case(C, dtype)
    coef[1], coef[C + 1] = 1.0, 0.1  # no tiny channel here: the changed element is an ordinary one
    out = nm.bn_apply_emul(y, coef, None, None, C, 0, False).to(dtype)
    _, ref, mag = nm.bn_apply_ref(y, coef, None, None, C, 0, False)
    nm.assert_rounded(out, ref, mag, dtype, C=C)
    # an element in the lower part of its binade (where one ulp is furthest above the half-ulp bound)
    frac = torch.frexp(ref.abs().float())[0]
    i = int(((frac > 0.5) & (frac < 0.6) & (ref.abs() > 0.1)).flatten().nonzero()[0])
    bad = out.clone().flatten()
    bits = bad.view(torch.int16)
    # the neighbouring representable value on the side away from the reference: one ulp from the correct rounding
    up = float((bits[i:i + 1] + 1).view(dtype).double().item())
    down = float((bits[i:i + 1] - 1).view(dtype).double().item())
    r = float(ref.flatten()[i].item())
    bits[i] += 1 if abs(up - r) > abs(down - r) else -1
    with pytest.raises(AssertionError, match=f"worst element {i}, channel {i % C}"):
        nm.assert_rounded(bad.view_as(out), ref, mag, dtype, C=C)


@pytest.mark.parametrize("dtype", DTYPES)
def test_assert_rounded_rejects_coefficients_shifted_by_one_channel(dtype):
    C = 64
    y, res, coef, rcoef = _apply_case(C, dtype)
    _, ref, mag = nm.bn_apply_ref(y, coef, res, rcoef, C, 2, True)
    shifted = torch.cat([coef[:C].roll(1), coef[C:2 * C].roll(1), coef[2 * C:]])
    out = nm.bn_apply_emul(y, shifted, res, rcoef, C, 2, True).to(dtype)
    with pytest.raises(AssertionError, match="out of bound"):
        nm.assert_rounded(out, ref, mag, dtype, C=C)
    b = torch.randn(3 * C, generator=torch.Generator().manual_seed(1))
    refb, magb = nm.bn_bwd_apply_ref(res.double(), y, b, C)
    outb = (b[:C].roll(1) * res.float() + b[C:2 * C].roll(1) * y.float() + b[2 * C:].roll(1)).to(dtype)
    with pytest.raises(AssertionError, match="out of bound"):
        nm.assert_rounded(outb, refb, magb, dtype, C=C)


@pytest.mark.parametrize("dtype", DTYPES)
def test_assert_sum_rejects_one_missing_row(dtype):
    rows, C, blocks, rpi = 3000, 128, 12, 16
    dz, y, mean, invstd = _reduce_case(rows, C, dtype)
    s0, s1, m0, m1 = _reduce_ref(dz, y, mean, invstd)
    n_chain = math.ceil(rows / (blocks * rpi)) + rpi
    nm.assert_sum(s0, s0, m0, n_chain)
    a0, a1, _, _ = _reduce_ref(dz[:-1], y[:-1], mean, invstd)
    with pytest.raises(AssertionError, match="out of bound"):
        nm.assert_sum(a0, s0, m0, n_chain, C=C)
    with pytest.raises(AssertionError, match="out of bound"):
        nm.assert_sum(a1, s1, m1, n_chain, C=C)


def test_assert_within_rejects_nan_and_names_the_channel():
    ref = torch.ones(4, 8, dtype=torch.float64)
    got = ref.clone()
    got[2, 5] = float("nan")
    with pytest.raises(AssertionError, match="worst element 21, channel 5"):
        nm.assert_within(got, ref, torch.full_like(ref, 1e-3), C=8)


def test_backward_reference_formula_equals_autograd_fp64():
    g = torch.Generator().manual_seed(7)
    rows, C, eps = 517, 64, 1e-5
    y = (torch.randn(rows, C, generator=g, dtype=torch.float64) * 1.7 + 0.4).requires_grad_(True)
    gamma = (torch.rand(C, generator=g, dtype=torch.float64) + 0.5).requires_grad_(True)
    beta = torch.randn(C, generator=g, dtype=torch.float64).requires_grad_(True)
    dz = torch.randn(rows, C, generator=g, dtype=torch.float64)
    F.batch_norm(y, None, None, gamma, beta, True, 0.1, eps).backward(dz)
    yd = y.detach()
    mean = yd.mean(0)
    invstd = 1.0 / torch.sqrt(yd.var(0, unbiased=False) + eps)
    xh = (yd - mean) * invstd
    sdz, sdzx = dz.sum(0), (dz * xh).sum(0)
    A = gamma.detach() * invstd
    B = -A * invstd * sdzx / rows
    Cc = -A * sdz / rows + A * invstd * (sdzx / rows) * mean
    dy = A * dz + B * yd + Cc
    assert (dy - y.grad).abs().max().item() < 1e-10
    assert (sdzx - gamma.grad).abs().max().item() < 1e-10
    assert (sdz - beta.grad).abs().max().item() < 1e-10
    # nm.bn_bwd_finalize_ref is that formula
    coef = torch.cat([A, beta.detach() - mean * A, mean, invstd])
    r = nm.bn_bwd_finalize_ref(sdz, sdzx, float(rows), coef, gamma.detach(), 1.0, C)
    assert (r["A"] * dz + r["B"] * yd + r["Cc"] - y.grad).abs().max().item() < 1e-10
