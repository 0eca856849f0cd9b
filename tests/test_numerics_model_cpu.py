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


# =================================================================================== the conv error model (16-bit MFMA)
# The reference alone; two correct fp32 implementations inside the bounds; ten mutations of a correct result, each on
# ONE element (at a ragged-tail row and at an image-corner pixel), rejected by the assertion that owns them.
import _conv_cases as cc  # noqa: E402


def _ref_of(kind, g, dtype, layer, opt):
    if kind == "fwd":
        x, w, _ = cc.fwd_operands(g, dtype, layer, narrow=g in cc.NARROW)
        return nm.conv_fwd_ref(x, w, g[6], g[7]) + (g[4],)
    if kind == "fwd_pre":
        z, w, _ = cc.fwd_operands(g, dtype, layer)
        a = cc.pre_apply_ref(z, cc.pre_operands(layer, dtype), dtype).float().to(dtype)
        return nm.conv_fwd_ref(a, w, g[6], g[7]) + (g[4],)
    if kind == "stem":
        x, wk = cc.stem_operands(g[0], g[1], g[2], dtype, layer)
        return nm.conv_fwd_ref(x.to(dtype).permute(0, 2, 3, 1), wk, 2, 3) + (64,)
    if kind == "first":
        x, wk, _ = cc.first_conv_operands((g[5], g[6], g[7], g[0], g[1], g[2]), dtype, layer)
        return nm.conv_fwd_ref(x.to(dtype).permute(0, 2, 3, 1), wk, g[6], g[7]) + (64,)
    if kind.startswith("grouped"):
        _, _, full = cc.grouped_weights(g[3], opt["groups"], dtype, layer)
        if kind == "grouped_fwd":
            return nm.conv_fwd_ref(cc.fwd_operands(g, dtype, layer)[0], full, g[6], g[7]) + (g[4],)
        return nm.conv_dgrad_ref(cc.dgrad_operands(g, dtype, layer)[0], full, g[1], g[2], g[6], g[7]) + (g[3],)
    dy, w, res = cc.dgrad_operands(g, dtype, layer, opt["residual"], narrow=g in cc.NARROW)
    return nm.conv_dgrad_ref(dy, w, g[1], g[2], g[6], g[7], res, (0, 0) if opt["residual"] == "compact" else None) \
        + (g[3],)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind,g,opt", cc.layer_a_cases(), ids=lambda v: str(v).replace(" ", ""))
def test_layer_a_cases_stay_exactly_representable(kind, g, opt, dtype):
    """At most 1 % of a case's outputs outside the dtype's exact integer range, every per-channel sum of squares below
    2**24 (the statistics stay exact), and mag -- the bound on every partial sum -- below 2**24 (so does the
    accumulator)."""
    ref, mag, K = _ref_of(kind, g, dtype, "int", opt)
    share, sumsq = nm.int_case_conditions(ref, dtype, K)
    assert share <= 0.01, share
    assert sumsq < 2.0 ** 24, sumsq
    assert float(mag.max()) < 2.0 ** 24
    assert bool((ref == ref.round()).all()) and bool((ref != 0).any())


def test_layer_a_plain_fp32_conv_is_exact():
    g = (2, 15, 13, 64, 128, 3, 2, 1)
    x, w, _ = cc.fwd_operands(g, torch.bfloat16, "int")
    ref, _ = nm.conv_fwd_ref(x, w, 2, 1)
    y = F.conv2d(x.float().permute(0, 3, 1, 2), w.float().permute(0, 3, 1, 2), stride=2, padding=1).permute(0, 2, 3, 1)
    assert torch.equal(y.double(), ref)
    dy, w, res = cc.dgrad_operands(g, torch.bfloat16, "int", "compact")
    refd, _ = nm.conv_dgrad_ref(dy, w, 15, 13, 2, 1, res, (0, 0))
    dx = torch.nn.grad.conv2d_input((2, 64, 15, 13), w.float().permute(0, 3, 1, 2), dy.float().permute(0, 3, 1, 2),
                                    stride=2, padding=1).permute(0, 2, 3, 1).clone()
    dx[:, ::2, ::2] += res.float()
    assert torch.equal(dx.double(), refd)
    xw, dyw = cc.wgrad_operands(g, torch.bfloat16, "int")
    refw, _ = nm.conv_wgrad_ref(xw, dyw, 3, 3, 2, 1)
    dw = torch.nn.grad.conv2d_weight(xw.float().permute(0, 3, 1, 2), (128, 64, 3, 3), dyw.float().permute(0, 3, 1, 2),
                                     stride=2, padding=1).permute(0, 2, 3, 1)
    assert torch.equal(dw.double(), refw)


def _grouped_sum(a, b, dim_terms, chunk=32, splits=3):
    """fp32 a @ b with the reduction axis evaluated adversarially: 32-term chunks summed first, the chunks of a split
    accumulated in reverse order, the split-K partials summed last (in reverse as well)."""
    T = dim_terms
    edges = list(range(0, T, chunk)) + [T]
    chunks = list(zip(edges[:-1], edges[1:]))
    per = -(-len(chunks) // splits)
    parts = []
    for s0 in range(0, len(chunks), per):
        acc = None
        for lo, hi in reversed(chunks[s0:s0 + per]):
            p = torch.matmul(a[..., lo:hi], b[..., lo:hi, :])
            acc = p if acc is None else acc + p
        parts.append(acc)
    total = parts[-1]
    for p in reversed(parts[:-1]):
        total = total + p
    return total


EMUL_GEOMS = cc.DEFAULT_GEOMS[:5] + [cc.PP_GEOMS[2], cc.c64_geom(421)]


def _record(family, worst, dtype):
    key = f"{family}/{str(dtype).split('.')[-1]}"
    nm.RATIOS[key] = max(nm.RATIOS.get(key, 0.0), worst)
    assert worst <= 1.0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("g", EMUL_GEOMS, ids=str)
def test_fp32_emulations_of_the_convs_stay_within_the_bounds(g, dtype):
    """Plain torch fp32 conv / conv2d_input / conv2d_weight and the adversarially grouped fp32 evaluation, on the
    layer-B operands: inside the bounds, ratios recorded (families cpu_*)."""
    N, H, W, C, K, R, st, pad = g
    P, Q = cc.out_hw(g)
    nchw = lambda t: t.float().permute(0, 3, 1, 2)
    # forward (+ residual, added in fp32 before the rounding)
    x, w, res = cc.fwd_operands(g, dtype, "real", residual=True)
    ref, mag = nm.conv_fwd_ref(x, w, st, pad, res)
    plain = F.conv2d(nchw(x), nchw(w), stride=st, padding=pad).permute(0, 2, 3, 1) + res.float()
    _record("cpu_plain_conv16_fwd",
            nm.assert_conv(plain.to(dtype), ref, mag, C * R * R, dtype, "plain fwd", None), dtype)
    cols = F.unfold(nchw(x), (R, R), padding=pad, stride=st)
    wm = nchw(w).reshape(K, C * R * R)
    grp = _grouped_sum(wm, cols, C * R * R).view(N, K, P, Q).permute(0, 2, 3, 1) + res.float()
    _record("cpu_grouped_conv16_fwd",
            nm.assert_conv(grp.to(dtype), ref, mag, C * R * R, dtype, "grouped fwd", None), dtype)
    if dtype == torch.float16:
        assert float(ref[..., 1].abs().max()) < 0.05  # the small channel
    # statistics of the rounded outputs, fp32 chain
    y = plain.to(dtype)
    yf = y.float().reshape(-1, K)
    s, ss = torch.zeros(K), torch.zeros(K)
    for r in range(yf.shape[0]):
        s, ss = s + yf[r], ss + yf[r] * yf[r]
    _record("cpu_plain_conv16_stats", nm.assert_conv_stats(s, ss, y, "stats chain", family=None), dtype)
    # data gradient
    dy, w, res = cc.dgrad_operands(g, dtype, "real", "full")
    ref, mag = nm.conv_dgrad_ref(dy, w, H, W, st, pad, res)
    plain = torch.nn.grad.conv2d_input((N, C, H, W), nchw(w), nchw(dy), stride=st, padding=pad).permute(0, 2, 3, 1) \
        + res.float()
    _record("cpu_plain_conv16_dgrad",
            nm.assert_conv(plain.to(dtype), ref, mag, K * R * R, dtype, "plain dgrad", None), dtype)
    dil, wt = nm.dgrad_as_correlation(dy, w, H, W, st, pad, torch.float32)
    grp = _grouped_sum(wt, F.unfold(dil, (R, R)), K * R * R).view(N, C, H, W).permute(0, 2, 3, 1) + res.float()
    _record("cpu_grouped_conv16_dgrad",
            nm.assert_conv(grp.to(dtype), ref, mag, K * R * R, dtype, "grouped dgrad", None), dtype)
    # weight gradient
    x, dy = cc.wgrad_operands(g, dtype, "real")
    ref, mag = nm.conv_wgrad_ref(x, dy, R, R, st, pad)
    plain = torch.nn.grad.conv2d_weight(nchw(x), (K, C, R, R), nchw(dy), stride=st, padding=pad).permute(0, 2, 3, 1)
    _record("cpu_plain_conv16_wgrad",
            nm.assert_conv(plain, ref, mag, N * P * Q, torch.float32, "plain wgrad", None), dtype)
    cols = F.unfold(nchw(x), (R, R), padding=pad, stride=st).permute(1, 0, 2).reshape(C * R * R, N * P * Q)
    grp = _grouped_sum(cols, dy.float().reshape(N * P * Q, K), N * P * Q)  # [C*R*R, K]
    grp = grp.view(C, R, R, K).permute(3, 1, 2, 0)
    _record("cpu_grouped_conv16_wgrad",
            nm.assert_conv(grp, ref, mag, N * P * Q, torch.float32, "grouped wgrad", None), dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", [1, 2, 3])
def test_fp32_emulation_of_the_fused_bn_backward_sums_stays_within_the_bound(mode, dtype):
    g = (2, 14, 14, 64, 64, 3, 1, 1)
    N, H, W, C, K, R, st, pad = g
    dy, w, res = cc.dgrad_operands(g, dtype, "real", None if mode == 1 else "full")
    ref, mag = nm.conv_dgrad_ref(dy, w, H, W, st, pad, res)
    d = cc.bnb_operands(mode, (N, H, W, C), dtype, "real")
    mask, unsure = cc.bnb_mask(mode, d, C)
    assert float(unsure.double().mean()) <= 1e-3
    plain = torch.nn.grad.conv2d_input((N, C, H, W), w.float().permute(0, 3, 1, 2), dy.float().permute(0, 3, 1, 2),
                                       stride=st, padding=pad).permute(0, 2, 3, 1)
    if res is not None:
        plain = plain + res.float()
    if mode == 1:
        m32 = (d["y1"].float().view(-1, C) * d["coef1"][:C] + d["coef1"][C:2 * C]) > 0
    else:
        m32 = mask
    dz = torch.where(m32, plain.reshape(-1, C), torch.zeros(())).to(dtype)
    ref2 = torch.where(mask, ref.reshape(-1, C), torch.zeros((), dtype=torch.float64))
    full = nm.conv_bound(ref, mag, K * R * R, dtype).reshape(-1, C)
    bound = torch.where(mask, full, torch.zeros_like(full))
    sb = torch.where(unsure, ref.reshape(-1, C).abs() + full, bound)
    for k in (1, 2) if mode == 3 else (1,):
        yk, ck = d[f"y{k}"], d[f"coef{k}"]
        xh32 = (yk.float().view(-1, C) - ck[2 * C:3 * C]) * ck[3 * C:]
        s0, s1 = torch.zeros(C), torch.zeros(C)
        for r in range(dz.shape[0]):
            s0, s1 = s0 + dz[r].float(), s1 + dz[r].float() * xh32[r]
        worst = nm.assert_bnb_sums(s0, s1, ref2, sb, nm.bn_xhat(yk, ck, C), f"branch {k}", family=None)
        _record("cpu_plain_conv16_bnb_sums", worst, dtype)


# ---- mutations
def _terms(x, w, n, p, q, k, st, pad):
    """fp64 products [C, R, S] of output element (n, p, q, k) (zero where the tap is padding)."""
    _, H, W, C = x.shape
    _, R, S, _ = w.shape
    t = torch.zeros(C, R, S, dtype=torch.float64)
    xin = torch.zeros(C, R, S, dtype=torch.float64)
    for r in range(R):
        for s in range(S):
            h, ww = p * st - pad + r, q * st - pad + s
            if 0 <= h < H and 0 <= ww < W:
                xin[:, r, s] = x[n, h, ww].double()
                t[:, r, s] = xin[:, r, s] * w[k, r, s].double()
    return t, xin


def _round16(v, dtype):
    return torch.tensor(v, dtype=torch.float64).float().to(dtype)


def _positions(ref, N, P, Q):
    """(ragged-tail row, image-corner pixel): the last-but-one pixel row of the GEMM and pixel (0, 0, 0); the channel is
    the one of median |ref| at that pixel: an ordinary element, inside every exact integer range and not one of the
    few whose terms cancel (there the accumulation term of the bound outweighs a 16-bit ulp, rightly)."""
    out = []
    for (n, p, q) in ((N - 1, P - 1, Q - 2), (0, 0, 0)):
        a = ref[n, p, q].abs()
        k = int((a - a.median()).abs().argmin())
        out.append((n, p, q, k))
    return out


def _expect_reject(layer, out, ref, mag, n_red, dtype):
    with pytest.raises(AssertionError, match="out of bound"):
        if layer == "int":
            nm.assert_exact(out, nm.round_exact(ref, dtype), "mutated")
        else:
            nm.assert_conv(out, ref, mag, n_red, dtype, "mutated", None)


def _accept(layer, out, ref, mag, n_red, dtype):
    if layer == "int":
        nm.assert_exact(out, nm.round_exact(ref, dtype), "correct")
    else:
        nm.assert_conv(out, ref, mag, n_red, dtype, "correct", None)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layer", ["int", "real"])
def test_element_assertions_reject_a_dropped_tap_channel_and_a_neighbouring_channel(layer, dtype):
    """Mutations 1-3 on one element of a 3x3 64 -> 64 forward."""
    g = (2, 14, 14, 64, 64, 3, 1, 1)
    N, H, W, C, K, R, st, pad = g
    x, w, _ = cc.fwd_operands(g, dtype, layer)
    ref, mag = nm.conv_fwd_ref(x, w, st, pad)
    good = F.conv2d(x.float().permute(0, 3, 1, 2), w.float().permute(0, 3, 1, 2), padding=pad).permute(0, 2, 3, 1)
    good = good.to(dtype)
    _accept(layer, good, ref, mag, C * 9, dtype)
    for (n, p, q, k) in _positions(ref, N, H, W):
        t, xin = _terms(x, w, n, p, q, k, st, pad)
        assert abs(float(t.sum()) - float(ref[n, p, q, k])) < 1e-9
        drop_tap = t.clone()
        drop_tap[:, 1, 1] = 0  # the centre tap is inside the image at every pixel
        # (integer terms can cancel: take the first channel whose contribution, or whose exchange, is not zero)
        c0 = next(c for c in range(5, C) if float(t[c].sum()) != 0)
        drop_ch = t.clone()
        drop_ch[c0] = 0
        c1 = next(c for c in range(5, C - 1) if float((xin[c + 1] * w[k, :, :, c].double() - t[c]).sum()) != 0)
        neigh = t.clone()
        neigh[c1] = xin[c1 + 1] * w[k, :, :, c1].double()
        for m in (drop_tap, drop_ch, neigh):
            bad = good.clone()
            bad[n, p, q, k] = _round16(float(m.sum()), dtype)
            _expect_reject(layer, bad, ref, mag, C * 9, dtype)


def _step_ulp(t16, away_from):
    """The neighbouring representable value of the one-element 16-bit tensor on the side away from ``away_from``."""
    bits = t16.clone().view(torch.int16)
    up, down = (bits + 1).view(t16.dtype), (bits - 1).view(t16.dtype)
    return up if abs(float(up) - away_from) > abs(float(down) - away_from) else down


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layer", ["int", "real"])
def test_element_assertions_reject_one_ulp_and_truncation_at_64_terms(layer, dtype):
    """Mutations 4 and 5 on the 64-term 1x1 conv, where the half-ulp term dominates the bound."""
    g = (2, 12, 12, 64, 256, 1, 1, 0)
    N, H, W, C, K, R, st, pad = g
    x, w, _ = cc.fwd_operands(g, dtype, layer)
    ref, mag = nm.conv_fwd_ref(x, w, st, pad)
    acc = F.conv2d(x.float().permute(0, 3, 1, 2), w.float().permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
    good = acc.to(dtype)
    _accept(layer, good, ref, mag, C, dtype)
    for (n, p, q, k) in _positions(ref, N, H, W):
        bad = good.clone()
        bad[n, p, q, k] = _step_ulp(good[n, p, q, k].reshape(1), float(ref[n, p, q, k]))[0]
        _expect_reject(layer, bad, ref, mag, C, dtype)
        if layer == "int":
            continue  # (integers are exact: there is nothing to truncate)
        # truncation: the 16-bit value next towards zero wherever rounding to nearest went away from zero
        row = good[n, p, q]
        went_up = row.double().abs() > acc[n, p, q].double().abs()
        bits = row.clone().view(torch.int16)
        trunc = torch.where(went_up, bits - 1, bits).view(dtype)  # sign-magnitude: -1 on the bits is towards zero
        bound = nm.conv_bound(ref[n, p, q], mag[n, p, q], C, dtype)
        ratio = (trunc.double() - ref[n, p, q]).abs() / bound
        kk = int(ratio.argmax())
        assert float(ratio[kk]) > 1.0
        bad = good.clone()
        bad[n, p, q, kk] = trunc[kk]
        _expect_reject(layer, bad, ref, mag, C, dtype)
    if layer == "real":  # and truncation everywhere
        bits = good.clone().view(torch.int16)
        trunc = torch.where(good.double().abs() > acc.double().abs(), bits - 1, bits).view(dtype)
        _expect_reject(layer, trunc, ref, mag, C, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layer", ["int", "real"])
def test_element_assertions_reject_a_doubled_and_a_misplaced_residual(layer, dtype):
    """Mutations 6 and 7 on a strided data gradient."""
    g = (2, 15, 13, 64, 128, 3, 2, 1)
    N, H, W, C, K, R, st, pad = g
    nchw = lambda t: t.float().permute(0, 3, 1, 2)
    dy, w, res = cc.dgrad_operands(g, dtype, layer, "full")
    ref, mag = nm.conv_dgrad_ref(dy, w, H, W, st, pad, res)
    plain = torch.nn.grad.conv2d_input((N, C, H, W), nchw(w), nchw(dy), stride=st, padding=pad).permute(0, 2, 3, 1)
    good = (plain + res.float()).to(dtype)
    _accept(layer, good, ref, mag, K * 9, dtype)
    for (n, p, q, k) in _positions(ref, N, H, W):
        bad = good.clone()
        bad[n, p, q, k] = (plain[n, p, q, k] + 2 * res[n, p, q, k].float()).to(dtype)
        _expect_reject(layer, bad, ref, mag, K * 9, dtype)
    # compact residual of phase (0, 0) placed on phase (0, 1) instead: one element of the wrong tensor
    dy, w, rc = cc.dgrad_operands(g, dtype, layer, "compact")
    ref, mag = nm.conv_dgrad_ref(dy, w, H, W, st, pad, rc, (0, 0))
    good = plain.clone()
    good[:, ::2, ::2] += rc.float()
    good = good.to(dtype)
    _accept(layer, good, ref, mag, K * 9, dtype)
    wrong = plain.clone()
    wrong[:, ::2, 1::2] += rc.float()[:, :, :W // 2]
    wrong = wrong.to(dtype)
    for (n, p, q) in ((N - 1, H - 1, W - 1), (0, 0, 0), (0, 0, 1)):  # two pixels that lose it, one that gains it
        bad = good.clone()
        bad[n, p, q, 7] = wrong[n, p, q, 7]
        _expect_reject(layer, bad, ref, mag, K * 9, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layer", ["int", "real"])
def test_statistics_assertion_rejects_one_missing_row(layer, dtype):
    """Mutation 8."""
    g = (2, 14, 14, 64, 64, 3, 1, 1)
    x, w, _ = cc.fwd_operands(g, dtype, layer)
    y = F.conv2d(x.float().permute(0, 3, 1, 2), w.float().permute(0, 3, 1, 2), padding=1).permute(0, 2, 3, 1).to(dtype)
    y64 = y.double().reshape(-1, 64)
    s, ss = y64.sum(0), (y64 * y64).sum(0)
    nm.assert_conv_stats(s, ss, y, "correct", family=None, exact=layer == "int")
    for row in (y64.shape[0] - 2, 0):
        with pytest.raises(AssertionError, match="out of bound"):
            nm.assert_conv_stats(s - y64[row], ss, y, "sum", family=None, exact=layer == "int")
        with pytest.raises(AssertionError, match="out of bound"):
            nm.assert_conv_stats(s, ss - y64[row] ** 2, y, "sumsq", family=None, exact=layer == "int")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layer", ["int", "real"])
def test_bn_backward_sums_assertion_rejects_branch_1_coefficients_on_branch_2(layer, dtype):
    """Mutation 9, and the sums of a dz that is wrong in one element (what a reference taken from the kernel's own
    output could never see)."""
    g = (2, 14, 14, 64, 64, 3, 1, 1)
    N, H, W, C, K, R, st, pad = g
    dy, w, res = cc.dgrad_operands(g, dtype, layer, "full")
    ref, mag = nm.conv_dgrad_ref(dy, w, H, W, st, pad, res)
    d = cc.bnb_operands(3, (N, H, W, C), dtype, layer)
    mask, _ = cc.bnb_mask(3, d, C)
    ref2 = torch.where(mask, ref.reshape(-1, C), torch.zeros((), dtype=torch.float64))
    full = nm.conv_bound(ref, mag, K * 9, dtype).reshape(-1, C)
    bound = torch.where(mask, full, torch.zeros_like(full))
    exact = layer == "int"
    dz = nm.round_exact(ref2, dtype)  # a correct kernel's dz (correctly rounded)
    x1, x2 = nm.bn_xhat(d["y1"], d["coef1"], C), nm.bn_xhat(d["y2"], d["coef2"], C)
    want = dz if exact else ref2
    nm.assert_bnb_sums(dz.sum(0), (dz * x2).sum(0), want, bound, x2, "correct", family=None, exact=exact)
    with pytest.raises(AssertionError, match="out of bound"):
        nm.assert_bnb_sums(dz.sum(0), (dz * x1).sum(0), want, bound, x2, "branch 2", family=None, exact=exact)
    # y2 read with branch 1's mean / invstd
    c12 = torch.cat([d["coef2"][:2 * C], d["coef1"][2 * C:]])
    with pytest.raises(AssertionError, match="out of bound"):
        nm.assert_bnb_sums(dz.sum(0), (dz * nm.bn_xhat(d["y2"], c12, C)).sum(0), want, bound, x2, "branch 2",
                           family=None, exact=exact)
    # one element of dz without one term, summed consistently: the exact layer sees it in the sums as well (in the
    # real layer a single term is below the sums' bound and is the element assertion's to catch)
    if not exact:
        return
    rows = dz.shape[0]
    for row in (rows - 2, 0):
        k = int(mask[row].double().argmax())
        bad = dz.clone()
        bad[row, k] = float(_round16(float(ref2[row, k] - dy[row // (H * W), (row // W) % H, row % W, 5].double()
                                           * w[5, 1, 1, k].double()), dtype))
        assert bad[row, k] != dz[row, k]
        with pytest.raises(AssertionError, match="out of bound"):
            nm.assert_bnb_sums(bad.sum(0), (bad * x1).sum(0), want, bound, x1, "branch 1", family=None, exact=exact)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layer", ["int", "real"])
def test_element_assertion_rejects_a_value_from_another_group_slice(layer, dtype):
    """Mutation 10: one output of slice 0 holds slice 1's value at the same pixel."""
    width, groups, stride, H = cc.GROUPED[0]
    g = cc.grouped_geom(width, groups, stride, H)
    _, _, full = cc.grouped_weights(width, groups, dtype, layer)
    x, _, _ = cc.fwd_operands(g, dtype, layer)
    ref, mag = nm.conv_fwd_ref(x, full, stride, 1)
    good = F.conv2d(x.float().permute(0, 3, 1, 2), full.float().permute(0, 3, 1, 2), stride=stride,
                    padding=1).permute(0, 2, 3, 1).to(dtype)
    _accept(layer, good, ref, mag, 64 * 9, dtype)
    P, Q = cc.out_hw(g)
    for (n, p, q) in ((1, P - 1, Q - 2), (0, 0, 0)):
        k = next(k for k in range(64) if good[n, p, q, k] != good[n, p, q, k + 64])
        bad = good.clone()
        bad[n, p, q, k] = good[n, p, q, k + 64]
        _expect_reject(layer, bad, ref, mag, 64 * 9, dtype)


# =================================================================================== the fp32 conv error model (fp32 MFMA)
# The same proofs for dtype float32 (tests/test_conv32_numerics_gpu.py): the integer cases are exact, two correct fp32
# evaluations stay inside the real bound, the assertions reject the mutations, and the ``wide`` layer holds the width of
# the multiply.
F32 = torch.float32
_nchw = lambda t: t.float().permute(0, 3, 1, 2)  # noqa: E731


def _rec32(family, worst):
    nm.RATIOS[family] = max(nm.RATIOS.get(family, 0.0), worst)
    assert worst <= 1.0


@pytest.mark.parametrize("kind,g,opt", cc.layer_a_cases32(), ids=lambda v: str(v).replace(" ", ""))
def test_layer_a32_cases_are_exact_and_plain_fp32_equals_fp64(kind, g, opt):
    """max |mag| < 2**24 (every partial sum is an exact integer), every per-channel sum of squares of the outputs below
    2**24 (the statistics are exact), and a plain torch fp32 evaluation equals the fp64 reference."""
    N, H, W, C, K, R, st, pad = g
    if kind == "fwd":
        x, w, res = cc.fwd_operands(g, F32, "int", residual=True)
        ref, mag = nm.conv_fwd_ref(x, w, st, pad, res)
        plain = F.conv2d(_nchw(x), _nchw(w), stride=st, padding=pad).permute(0, 2, 3, 1) + res
        ch = K
    elif kind == "dgrad":
        dy, w, res = cc.dgrad_operands(g, F32, "int", "full")
        ref, mag = nm.conv_dgrad_ref(dy, w, H, W, st, pad, res)
        plain = torch.nn.grad.conv2d_input((N, C, H, W), _nchw(w), _nchw(dy), stride=st, padding=pad).permute(0, 2, 3, 1) \
            + res
        ch = C
    elif kind == "wgrad":
        x, dy = cc.wgrad_operands(g, F32, "int")
        ref, mag = nm.conv_wgrad_ref(x, dy, R, R, st, pad)
        plain = torch.nn.grad.conv2d_weight(_nchw(x), (K, C, R, R), _nchw(dy), stride=st, padding=pad).permute(0, 2, 3, 1)
        ch = None
    else:
        x, w, dy = cc.stem32_operands(N, H, W, "int")
        ref, mag = nm.conv_fwd_ref(x.permute(0, 2, 3, 1), w, 2, 3)
        plain = F.conv2d(x, _nchw(w), stride=2, padding=3).permute(0, 2, 3, 1)
        ch = 64
        wref, wmag = nm.conv_wgrad_ref(x.permute(0, 2, 3, 1), dy, 7, 7, 2, 3)
        assert float(wmag.max()) < 2.0 ** 24
    assert float(mag.max()) < 2.0 ** 24
    if ch is not None:
        top, sumsq = nm.int32_case_conditions(ref, mag, ch)
        assert sumsq < 2.0 ** 24, sumsq
    assert bool((ref == ref.round()).all()) and bool((ref != 0).any())
    assert torch.equal(plain.double(), ref)


@pytest.mark.parametrize("g", [cc.C32_TILE_GEOM, cc.C32_TILE_GEOM_256] + [cc.dgrad_geom32(g) for g in cc.C32_HALO_GEOMS],
                         ids=str)
def test_layer_a32_fused_bn_backward_sums_are_exact_and_few_signs_are_uncertain(g):
    """The exact BN operands give sums in quarters below 2**22 (exact in fp32) with no uncertain sign; the real operands
    of the bn_mref = None epilogue leave out far less than 1 % of the elements."""
    N, H, W, C, K, R, st, pad = g
    for mode, res in ((1, None), (2, "full"), (3, "full")):
        dy, w, r = cc.dgrad_operands(g, F32, "int", res)
        ref, _ = nm.conv_dgrad_ref(dy, w, H, W, st, pad, r)
        d = cc.bnb_operands(mode, (N, H, W, C), F32, "int")
        mask, unsure = cc.bnb_mask(mode, d, C)
        assert not bool(unsure.any())
        dz = torch.where(mask, ref.reshape(-1, C), torch.zeros((), dtype=torch.float64))
        for k in (1, 2) if mode == 3 else (1,):
            xh = nm.bn_xhat(d[f"y{k}"], d[f"coef{k}"], C)
            assert float((dz * xh).abs().sum(0).max()) < 2.0 ** 22
            assert bool(((dz * xh * 4) == (dz * xh * 4).round()).all())
    _, unsure = cc.bnb_mask(1, cc.bnb_operands(1, (N, H, W, C), F32, "real"), C)
    assert float(unsure.double().mean()) < 0.01


EMUL32_GEOMS = cc.C32_DEFAULT_GEOMS[:5] + [cc.C32_HALO_GEOMS[3]]


@pytest.mark.parametrize("g", EMUL32_GEOMS, ids=str)
def test_fp32_emulations_of_the_fp32_convs_stay_within_the_bounds(g):
    """Plain torch fp32 and the adversarially grouped fp32 evaluation on the real operands: inside (n + 5)*2u*mag;
    ratios recorded as cpu_plain_conv32_* / cpu_grouped_conv32_*."""
    N, H, W, C, K, R, st, pad = g
    P, Q = cc.out_hw(g)
    x, w, res = cc.fwd_operands(g, F32, "real", residual=True)
    ref, mag = nm.conv_fwd_ref(x, w, st, pad, res)
    assert float(ref[..., 1].abs().max()) < 0.05  # the small channel
    plain = F.conv2d(_nchw(x), _nchw(w), stride=st, padding=pad).permute(0, 2, 3, 1) + res
    _rec32("cpu_plain_conv32_fwd", nm.assert_conv32(plain, ref, mag, C * R * R, "plain fwd", None))
    cols = F.unfold(_nchw(x), (R, R), padding=pad, stride=st)
    grp = _grouped_sum(_nchw(w).reshape(K, C * R * R), cols, C * R * R).view(N, K, P, Q).permute(0, 2, 3, 1) + res
    _rec32("cpu_grouped_conv32_fwd", nm.assert_conv32(grp, ref, mag, C * R * R, "grouped fwd", None))
    yf = plain.reshape(-1, K)
    s, ss = torch.zeros(K), torch.zeros(K)
    for r in range(yf.shape[0]):
        s, ss = s + yf[r], ss + yf[r] * yf[r]
    _rec32("cpu_plain_conv32_stats", nm.assert_conv_stats(s, ss, plain, "stats chain", family=None))
    gd = g if C % 64 == 0 else cc.dgrad_geom32(g)
    N, H, W, C, K, R, st, pad = gd
    dy, w, res = cc.dgrad_operands(gd, F32, "real", "full")
    ref, mag = nm.conv_dgrad_ref(dy, w, H, W, st, pad, res)
    plain = torch.nn.grad.conv2d_input((N, C, H, W), _nchw(w), _nchw(dy), stride=st, padding=pad).permute(0, 2, 3, 1) + res
    _rec32("cpu_plain_conv32_dgrad", nm.assert_conv32(plain, ref, mag, K * R * R, "plain dgrad", None))
    dil, wt = nm.dgrad_as_correlation(dy, w, H, W, st, pad, torch.float32)
    grp = _grouped_sum(wt, F.unfold(dil, (R, R)), K * R * R).view(N, C, H, W).permute(0, 2, 3, 1) + res
    _rec32("cpu_grouped_conv32_dgrad", nm.assert_conv32(grp, ref, mag, K * R * R, "grouped dgrad", None))
    N, H, W, C, K, R, st, pad = g
    x, dy = cc.wgrad_operands(g, F32, "real")
    ref, mag = nm.conv_wgrad_ref(x, dy, R, R, st, pad)
    plain = torch.nn.grad.conv2d_weight(_nchw(x), (K, C, R, R), _nchw(dy), stride=st, padding=pad).permute(0, 2, 3, 1)
    _rec32("cpu_plain_conv32_wgrad", nm.assert_conv32(plain, ref, mag, N * P * Q, "plain wgrad", None))
    cols = F.unfold(_nchw(x), (R, R), padding=pad, stride=st).permute(1, 0, 2).reshape(C * R * R, N * P * Q)
    grp = _grouped_sum(cols, dy.reshape(N * P * Q, K), N * P * Q).view(C, R, R, K).permute(3, 1, 2, 0)
    _rec32("cpu_grouped_conv32_wgrad", nm.assert_conv32(grp, ref, mag, N * P * Q, "grouped wgrad", None))


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_fp32_emulation_of_the_fp32_fused_bn_backward_sums_stays_within_the_bound(mode):
    g = (2, 14, 9, 64, 64, 3, 1, 1)
    N, H, W, C, K, R, st, pad = g
    dy, w, res = cc.dgrad_operands(g, F32, "real", None if mode == 1 else "full")
    ref, mag = nm.conv_dgrad_ref(dy, w, H, W, st, pad, res)
    d = cc.bnb_operands(mode, (N, H, W, C), F32, "real")
    mask, unsure = cc.bnb_mask(mode, d, C)
    plain = torch.nn.grad.conv2d_input((N, C, H, W), _nchw(w), _nchw(dy), stride=st, padding=pad).permute(0, 2, 3, 1)
    if res is not None:
        plain = plain + res
    m32 = (d["y1"].view(-1, C) * d["coef1"][:C] + d["coef1"][C:2 * C]) > 0 if mode == 1 else mask
    dz = torch.where(m32, plain.reshape(-1, C), torch.zeros(()))
    ref2 = torch.where(mask, ref.reshape(-1, C), torch.zeros((), dtype=torch.float64))
    full = nm.conv32_bound(mag, K * R * R).reshape(-1, C)
    sb = torch.where(unsure, ref.reshape(-1, C).abs() + full, torch.where(mask, full, torch.zeros_like(full)))
    for k in (1, 2) if mode == 3 else (1,):
        yk, ck = d[f"y{k}"], d[f"coef{k}"]
        xh32 = (yk.view(-1, C) - ck[2 * C:3 * C]) * ck[3 * C:]
        s0, s1 = torch.zeros(C), torch.zeros(C)
        for r in range(dz.shape[0]):
            s0, s1 = s0 + dz[r], s1 + dz[r] * xh32[r]
        _rec32("cpu_plain_conv32_bnb_sums",
               nm.assert_bnb_sums(s0, s1, ref2, sb, nm.bn_xhat(yk, ck, C), f"branch {k}", family=None))


def _stem_fused_cpu(N, H, W, layer):
    P, Q = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    x, _, _ = cc.stem32_operands(N, H, W, layer)
    d = cc.stem32_tail_operands(N, P, Q, layer)
    r = cc.stem_tail_ref(d, N, P, Q, 64)
    xh = x.permute(0, 2, 3, 1)
    ref, _ = nm.conv_wgrad_ref(xh, r["dy"], 7, 7, 2, 3)
    _, mag = nm.conv_wgrad_ref(xh, r["dymag"], 7, 7, 2, 3)
    _, flip = nm.conv_wgrad_ref(xh, r["dyflip"], 7, 7, 2, 3)
    return x, d, r, ref, mag, flip


@pytest.mark.parametrize("N,H,W", cc.STEM32_FUSED[:1] + cc.STEM32_FUSED[2:3])
def test_fp32_emulation_of_the_fused_stem_weight_gradient(N, H, W):
    """dY formed in fp32 (scatter, mask, A*dz + B*y + C) and torch's fp32 conv2d_weight: inside (n + 12)*2u*mag on the
    real operands and equal to the fp64 reference on the exact ones; a dY built from argmax codes shifted by one is
    rejected by both layers."""
    P, Q = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    for layer in ("int", "real"):
        x, d, r, ref, mag, flip = _stem_fused_cpu(N, H, W, layer)

        def emul(idx):
            r32 = cc.stem_tail_ref(dict(d, idx=idx), N, P, Q, 64)
            pre = d["y"] * d["coef"][:64] + d["coef"][64:128]
            dz = torch.where(pre > 0, r32["dzraw"].float(), torch.zeros(()))  # the fp32 mask on the rounded scatter
            dy = d["b"][:64] * dz + d["b"][64:128] * d["y"] + d["b"][128:192]
            return torch.nn.grad.conv2d_weight(x, (64, 3, 7, 7), _nchw(dy), stride=2, padding=3).permute(0, 2, 3, 1)
        bound = nm.conv32_bound(mag, N * P * Q, extra=12) + flip
        good, bad = emul(d["idx"]), emul((d["idx"] + 1) % 9)
        if layer == "int":
            assert not bool(r["unsure"].any()) and float(mag.max()) < 2.0 ** 23
            nm.assert_exact(good, ref, "stem fused emulation")
            with pytest.raises(AssertionError, match="out of bound"):
                nm.assert_exact(bad, ref, "shifted argmax")
        else:
            _rec32("cpu_plain_conv32_stem_fused", nm.assert_within(good, ref, bound, "stem fused emulation", 3, None))
            with pytest.raises(AssertionError, match="out of bound"):
                nm.assert_within(bad, ref, bound, "shifted argmax", 3, None)


def _check32(layer, out, ref, mag, n):
    if layer == "int":
        nm.assert_exact(out, ref, "case")
    else:
        nm.assert_conv32(out, ref, mag, n, "case", None)


@pytest.mark.parametrize("layer", ["int", "real"])
def test_fp32_element_assertions_reject_a_dropped_tap_a_neighbouring_channel_and_residual_mistakes(layer):
    g = (2, 14, 9, 64, 64, 3, 1, 1)
    N, H, W, C, K, R, st, pad = g
    x, w, res = cc.fwd_operands(g, F32, layer, residual=True)
    ref, mag = nm.conv_fwd_ref(x, w, st, pad, res)
    conv = F.conv2d(_nchw(x), _nchw(w), padding=pad).permute(0, 2, 3, 1)
    good = conv + res
    _check32(layer, good, ref, mag, C * 9)
    for (n, p, q, k) in _positions(ref, N, H, W) + [(1, 3, 4, 1)]:  # ... and the small channel
        t, xin = _terms(x, w, n, p, q, k, st, pad)
        r0 = float(res[n, p, q, k])
        assert abs(float(t.sum()) + r0 - float(ref[n, p, q, k])) < 1e-9
        drop_tap = t.clone()
        drop_tap[:, 1, 1] = 0
        c1 = next(c for c in range(5, C - 1) if float((xin[c + 1] * w[k, :, :, c].double() - t[c]).sum()) != 0)
        neigh = t.clone()
        neigh[c1] = xin[c1 + 1] * w[k, :, :, c1].double()
        q2 = q + 1 if q + 1 < W else q - 1
        for val in (float(drop_tap.sum()) + r0, float(neigh.sum()) + r0, float(t.sum()) + 2 * r0,
                    float(t.sum()) + float(res[n, p, q2, k])):  # dropped tap, neighbour, doubled / misplaced residual
            if val == float(ref[n, p, q, k]):
                continue  # (integer terms can cancel)
            bad = good.clone()
            bad[n, p, q, k] = val
            with pytest.raises(AssertionError, match="out of bound"):
                _check32(layer, bad, ref, mag, C * 9)
    # a transposed H / W in the reference is seen by a correct result (the inverted reference check)
    xt = x.transpose(1, 2).contiguous().view(N, H, W, C) if H != W else x
    rt, _ = nm.conv_fwd_ref(xt, w, st, pad, res)
    with pytest.raises(AssertionError, match="index"):
        _check32(layer, good, rt, mag, C * 9)


@pytest.mark.parametrize("layer", ["int", "real"])
def test_fp32_statistics_and_bn_backward_sum_assertions_reject_a_missing_row_and_swapped_branches(layer):
    g = (2, 14, 9, 64, 64, 3, 1, 1)
    N, H, W, C, K, R, st, pad = g
    exact = layer == "int"
    x, w, _ = cc.fwd_operands(g, F32, layer)
    y = F.conv2d(_nchw(x), _nchw(w), padding=1).permute(0, 2, 3, 1)
    y64 = y.double().reshape(-1, K)
    s, ss = y64.sum(0), (y64 * y64).sum(0)
    nm.assert_conv_stats(s, ss, y, "correct", family=None, exact=exact)
    for row in (y64.shape[0] - 2, 0):
        with pytest.raises(AssertionError, match="out of bound"):
            nm.assert_conv_stats(s - y64[row], ss, y, "sum", family=None, exact=exact)
        with pytest.raises(AssertionError, match="out of bound"):
            nm.assert_conv_stats(s, ss - y64[row] ** 2, y, "sumsq", family=None, exact=exact)
    dy, w, res = cc.dgrad_operands(g, F32, layer, "full")
    ref, mag = nm.conv_dgrad_ref(dy, w, H, W, st, pad, res)
    d = cc.bnb_operands(3, (N, H, W, C), F32, layer)
    mask, _ = cc.bnb_mask(3, d, C)
    dz = torch.where(mask, ref.reshape(-1, C), torch.zeros((), dtype=torch.float64))
    full = nm.conv32_bound(mag, K * 9).reshape(-1, C)
    bound = torch.where(mask, full, torch.zeros_like(full))
    x1, x2 = nm.bn_xhat(d["y1"], d["coef1"], C), nm.bn_xhat(d["y2"], d["coef2"], C)
    nm.assert_bnb_sums(dz.sum(0), (dz * x2).sum(0), dz, bound, x2, "correct", family=None, exact=exact)
    with pytest.raises(AssertionError, match="out of bound"):
        nm.assert_bnb_sums(dz.sum(0), (dz * x1).sum(0), dz, bound, x2, "branch 2", family=None, exact=exact)
    c12 = torch.cat([d["coef2"][:2 * C], d["coef1"][2 * C:]])
    with pytest.raises(AssertionError, match="out of bound"):
        nm.assert_bnb_sums(dz.sum(0), (dz * nm.bn_xhat(d["y2"], c12, C)).sum(0), dz, bound, x2, "branch 2", family=None,
                           exact=exact)
    with pytest.raises(AssertionError, match="out of bound"):  # one row missing from the fused sums
        nm.assert_bnb_sums((dz.sum(0) - dz[-2]), ((dz * x1).sum(0) - (dz * x1)[-2]), dz, bound, x1, "branch 1",
                           family=None, exact=exact)


@pytest.mark.parametrize("variant", cc.WIDE_VARIANTS)
def test_wide_layer_accepts_plain_fp32_and_rejects_19_bit_products_and_operands(variant):
    """Plain fp32 is exact on every ``wide`` case; a product rounded to 19 bits mismatches EVERY element of (a); an
    operand rounded to 19 bits on the 24-bit side mismatches every element of (b) and (c)."""
    g = cc.WIDE_FWD[1]
    N, H, W, C, K, R, st, pad = g
    x, w = cc.wide_fwd_operands(g, variant)
    ref, _ = nm.conv_fwd_ref(x, w, 1, 0)
    assert bool((ref != 0).all()) and bool((x != 0).sum(-1).eq(1).all())
    y = F.conv2d(_nchw(x), _nchw(w)).permute(0, 2, 3, 1)
    nm.assert_exact(y, ref, "plain fp32")
    if variant == "a":
        narrow = nm.round_to_bits(y, 19)
        assert bool((narrow.double() != ref).all())
    else:
        xs, ws = (nm.round_to_bits(x, 19), w) if variant == "b" else (x, nm.round_to_bits(w, 19))
        narrow = F.conv2d(_nchw(xs), _nchw(ws)).permute(0, 2, 3, 1)
        assert bool((narrow.double() != ref).all())
    with pytest.raises(AssertionError, match="out of bound"):
        nm.assert_exact(narrow, ref, "19 bits")
    gd = cc.dgrad_geom32(g)
    dy, wd = cc.wide_dgrad_operands(gd, variant)
    refd, _ = nm.conv_dgrad_ref(dy, wd, H, W, 1, 0)
    dx = torch.nn.grad.conv2d_input((N, K, H, W), _nchw(wd), _nchw(dy)).permute(0, 2, 3, 1)
    assert bool((refd != 0).all())
    nm.assert_exact(dx, refd, "plain fp32 dgrad")
    for gw, tile in cc.WIDE_WGRAD:
        xw, dyw = cc.wide_wgrad_operands(gw, variant)
        refw, _ = nm.conv_wgrad_ref(xw, dyw, 1, 1, 1, 0)
        assert bool((refw != 0).all())
        dw = torch.einsum("pc,pk->kc", xw.reshape(-1, gw[3]), dyw.reshape(-1, gw[4])).view(gw[4], 1, 1, gw[3])
        nm.assert_exact(dw, refw, "plain fp32 wgrad")
        with pytest.raises(AssertionError, match="out of bound"):
            nm.assert_exact(nm.round_to_bits(dw, 19) if variant == "a" else torch.einsum(
                "pc,pk->kc", nm.round_to_bits(xw, 19).reshape(-1, gw[3]),
                nm.round_to_bits(dyw, 19).reshape(-1, gw[4])).view(gw[4], 1, 1, gw[3]), refw, "19 bits")


def test_real_bound_at_32_terms_rejects_11_bit_operands_and_long_reductions_do_not():
    """The real layer owns scaling and rounding-mode errors, not the width of the multiply: at n = 32 operands rounded
    to 11 bits fail the bound, at n = 4608 even 8-bit operands pass it (hence the ``wide`` layer)."""
    g = cc.WIDE_FWD[0]
    x, w, _ = cc.fwd_operands(g, F32, "real")
    ref, mag = nm.conv_fwd_ref(x, w, 1, 0)
    nm.assert_conv32(F.conv2d(_nchw(x), _nchw(w)).permute(0, 2, 3, 1), ref, mag, 32, "plain", None)
    r11, _ = nm.conv_fwd_ref(nm.round_to_bits(x, 11), nm.round_to_bits(w, 11), 1, 0)
    with pytest.raises(AssertionError, match="out of bound"):
        nm.assert_conv32(r11, ref, mag, 32, "11-bit operands", None)
    g = (2, 8, 6, 512, 128, 3, 1, 1)
    x, w, _ = cc.fwd_operands(g, F32, "real")
    ref, mag = nm.conv_fwd_ref(x, w, 1, 1)
    r8, _ = nm.conv_fwd_ref(nm.round_to_bits(x, 8), nm.round_to_bits(w, 8), 1, 1)
    nm.assert_conv32(r8, ref, mag, 4608, "8-bit operands at n = 4608", None)


# ======================================================================= the 16-bit pools and stem tail (pool.hip)
# tests/test_stem_tail_numerics_gpu.py runs these assertions on the kernels; here a plain fp32 evaluation must pass them
# and the listed mutations must fail, and the conditions on the operands are checked from the references alone.
import _pool_cases as pc  # noqa: E402

POOL_SHAPES = [(1, 2, 12, 11, 64), (1, 2, 13, 11, 8), (0, 2, 13, 11, 64), (0, 2, 12, 10, 8), (0, 1, 3, 3, 8),
               (0, 1, 4, 4, 16), (0, 3, 27, 27, 192)]
TAIL_SHAPES = [(2, 12, 11, 64), (2, 13, 11, 64), (2, 55, 55, 64), (1, 3, 5, 64), (2, 13, 11, 8)]


def _tail_emul(d, N, P, Q, C, pad, dtype):
    """Plain fp32 evaluation of the backward tail: (dz of maxpool_bwd_relu, dY of stem_pool_bwd_apply, the [C, 2] sums of
    stem_pool_bwd_reduce), the first two rounded once to ``dtype``."""
    OH, OW = cc.pool_out_hw(P, Q, pad)
    idx = d["idx"]
    n_i, oh_i, ow_i, c_i = torch.meshgrid(*[torch.arange(s) for s in (N, OH, OW, C)], indexing="ij")
    h, w = oh_i * 2 - pad + (idx // 3).long(), ow_i * 2 - pad + (idx % 3).long()
    ok = (idx < 9) & (h >= 0) & (h < P) & (w >= 0) & (w < Q)
    acc = torch.zeros(N * P * Q * C)
    acc.index_put_(((((n_i * P + h) * Q + w) * C + c_i)[ok],), d["dp"].float()[ok], accumulate=True)
    yf = d["y"].float()
    coef, b = d["coef"], d["b"]
    dz = torch.where(yf * coef[:C] + coef[C:2 * C] > 0, acc.view(N, P, Q, C), torch.zeros(()))
    dy = b[:C] * dz + b[C:2 * C] * yf + b[2 * C:3 * C]
    xh = (yf - coef[2 * C:3 * C]) * coef[3 * C:4 * C]
    sums = torch.stack([dz.reshape(-1, C).sum(0), (dz * xh).reshape(-1, C).sum(0)], 1)
    return dz.to(dtype), dy.to(dtype), sums.double()


def _bump(t, ref, ok=None, exact=False):
    """``t`` with one element moved by one 16-bit ulp away from the reference: an element in the lower part of its binade
    (where one ulp is furthest above the half-ulp bound), as test_assert_rounded_rejects_one_element_off_by_one_ulp does;
    None where the case has no such element."""
    frac = torch.frexp(ref.abs().float())[0].flatten()
    pick = (frac > 0.5) & (frac < 0.6) & (ref.abs().flatten() > 2.0 ** -10)
    if exact:  # a zero bound: any element will do
        pick = ref.flatten() != 0
    if ok is not None:
        pick &= ok.flatten()
    if not bool(pick.any()):
        return None
    i = int(pick.nonzero()[0])
    bad = t.clone().flatten()
    bits = bad.view(torch.int16)
    up = float((bits[i:i + 1] + 1).view(t.dtype).double().item())
    down = float((bits[i:i + 1] - 1).view(t.dtype).double().item())
    r = float(ref.flatten()[i].item())
    bits[i] += 1 if abs(up - r) > abs(down - r) else -1
    return bad.view_as(t)


@pytest.mark.parametrize("dtype", cc.DTYPES)
@pytest.mark.parametrize("pad,N,H,W,C", POOL_SHAPES)
def test_fp32_emulation_of_the_pool_forward_passes_and_mutations_fail(pad, N, H, W, C, dtype):
    d = cc.stem_tail_operands(N, H, W, "real", dtype, C=C, pad=pad)
    r = pc.pool_fwd_ref(d["y"], d["coef"], 3, pad)
    out, idx = pc.pool_fwd_emul(d["y"], d["coef"], dtype, 3, pad, 255)
    assert pc.assert_pool_fwd(out, idx, r, dtype, 255, "emulation") <= 1.0
    bad = _bump(out, r["ref"])
    assert bad is not None or out.numel() <= 64
    if bad is not None:
        with pytest.raises(AssertionError, match="out"):
            pc.assert_pool_fwd(bad, idx, r, dtype, 255, "one ulp")
    # a dropped window member: the maximum without each window's first maximal member
    drop = r["win"].clone()
    drop.scatter_(-1, r["first"].unsqueeze(-1), -1.0)
    with pytest.raises(AssertionError, match="out"):
        pc.assert_pool_fwd(drop.max(-1).values.clamp_min(0).to(dtype), idx, r, dtype, 255, "dropped member")
    # an argmax shifted by one position in a decisive window
    live = r["decisive"].nonzero()
    if live.shape[0]:
        at = tuple(live[0].tolist())
        bad = idx.clone()
        bad[at] = (int(idx[at]) + 1) % 9
        with pytest.raises(AssertionError):
            pc.assert_pool_fwd(out, bad, r, dtype, 255, "argmax + 1")
    # coefficients shifted by one channel
    rolled = torch.cat([d["coef"][:C].roll(1), d["coef"][C:2 * C].roll(1), d["coef"][2 * C:]])
    o2, i2 = pc.pool_fwd_emul(d["y"], rolled, dtype, 3, pad, 255)
    with pytest.raises(AssertionError):
        pc.assert_pool_fwd(o2, i2, r, dtype, 255, "channel + 1")
    # a live window marked dead, a dead one marked live
    for mask, code in ((r["must_live"], 255), (r["must_dead"], 4)):
        hit = mask.nonzero()
        if hit.shape[0]:
            bad = idx.clone()
            bad[tuple(hit[0].tolist())] = code
            with pytest.raises(AssertionError):
                pc.assert_pool_fwd(out, bad, r, dtype, 255, "dead code")


@pytest.mark.parametrize("dtype", cc.DTYPES)
@pytest.mark.parametrize("pad,N,H,W,C", POOL_SHAPES)
def test_decisive_pool_planes_pin_every_output_and_argmax(pad, N, H, W, C, dtype):
    """The condition of the integer forward test, from the reference alone: every window is decisive or surely dead, the
    values are exactly representable, and the emulation is exact."""
    y, coef = pc.decisive_planes(N, H, W, C, H + C + pad)
    assert bool((y.to(dtype).float() == y).all())
    r = pc.pool_fwd_ref(y.to(dtype), coef, 3, pad)
    assert bool((r["decisive"] | r["must_dead"]).all()) and bool(r["must_dead"][..., 5].all()) and bool(r["decisive"].any())
    assert bool((nm.round_exact(r["ref"], dtype) == r["ref"]).all())
    out, idx = pc.pool_fwd_emul(y.to(dtype), coef, dtype, 3, pad, 255)
    pc.assert_pool_fwd(out, idx, r, dtype, 255, "emulation", exact=True)


@pytest.mark.parametrize("dtype", cc.DTYPES)
@pytest.mark.parametrize("layer", ["int", "real"])
@pytest.mark.parametrize("pad,N,H,W,C", POOL_SHAPES + [(1,) + s for s in TAIL_SHAPES])
def test_fp32_emulation_of_the_pool_backward_and_stem_tail(pad, N, H, W, C, layer, dtype):
    """maxpool_bwd_relu (both pads), stem_pool_bwd_apply and stem_pool_bwd_reduce (pad 1): the emulation passes, the
    unsure share is <= 1 %, the integer layer is exactly representable; one ulp16, a dropped window gradient, argmax
    bytes shifted by one and coefficients shifted by one channel fail."""
    exact = layer == "int"
    d = cc.stem_tail_operands(N, H, W, layer, dtype, C=C, pad=pad)
    r = cc.stem_tail_ref(d, N, H, W, C, pad)
    assert float(r["unsure"].double().mean()) <= 0.01
    dz, dy, sums = _tail_emul(d, N, H, W, C, pad, dtype)
    OH, OW = cc.pool_out_hw(H, W, pad)
    n_chain = pc.reduce16_plan(N * OH * OW, C, 4096)[2]
    if exact:
        assert not bool(r["unsure"].any())
        for v in (r["dz"], r["dy"]):
            assert bool((nm.round_exact(v, dtype) == v).all())
        assert float(r["dzmag"].reshape(-1, C).sum(0).max()) * 16 < 2 ** 24  # every sum of the reduce, in units of 1/16

    def check(dz_, dy_, sums_, rr, dd):
        pc.assert_pool_bwd(dz_, rr, dtype, "dz", exact=exact)
        if pad == 1:
            pc.assert_tail_apply(dy_, rr, dtype, "dy", exact=exact)
            pc.assert_tail_reduce(sums_, dd, rr, C, n_chain, "sums", exact=exact)

    check(dz, dy, sums, r, d)
    bad = _bump(dz, r["dz"], ~r["unsure"], exact)
    assert bad is not None or dz.numel() <= 256
    if bad is not None:
        with pytest.raises(AssertionError):
            pc.assert_pool_bwd(bad, r, dtype, "one ulp", exact=exact)
    if pad == 1:
        with pytest.raises(AssertionError):
            pc.assert_tail_apply(_bump(dy, r["dy"], ~r["unsure"], exact), r, dtype, "one ulp", exact=exact)
    # a dropped window gradient / argmax bytes shifted by one / coefficients of the neighbouring channel: the emulation
    # of the mutated operands against the reference of the true ones
    drop = dict(d, dp=d["dp"].clone())
    big = r["dz"].abs().clone()  # the pixel with the largest gradient outside the small channel
    big[..., 1] = 0
    n, h, w, c = [int(v) for v in torch.unravel_index(big.argmax(), big.shape)]
    for oh in range(OH):
        for ow in range(OW):
            k = int(d["idx"][n, oh, ow, c])
            if k < 9 and (oh * 2 - pad + k // 3, ow * 2 - pad + k % 3) == (h, w):
                drop["dp"][n, oh, ow, c] = 0
                break
        else:
            continue
        break
    shifted = dict(d, idx=torch.where(d["idx"] < 9, (d["idx"] + 1) % 9, d["idx"]))
    rolled = dict(d, coef=d["coef"].view(4, C).roll(1, 1).reshape(-1), b=d["b"].view(3, C).roll(1, 1).reshape(-1))
    for name, m in (("dropped window", drop), ("argmax + 1", shifted), ("channel + 1", rolled)):
        mdz, mdy, msums = _tail_emul(m, N, H, W, C, pad, dtype)
        if name != "channel + 1" or not exact or bool((mdz.double() != r["dz"]).any()):
            with pytest.raises(AssertionError):
                pc.assert_pool_bwd(mdz, r, dtype, name, exact=exact)
        if pad == 1:
            with pytest.raises(AssertionError):
                pc.assert_tail_apply(mdy, r, dtype, name, exact=exact)
            with pytest.raises(AssertionError):
                pc.assert_tail_reduce(msums, d, r, C, n_chain, name, exact=exact)


@pytest.mark.parametrize("dtype", cc.DTYPES)
@pytest.mark.parametrize("k,pad,N,H,W,C", [(3, 1, 2, 12, 11, 64), (3, 1, 2, 13, 11, 8), (3, 0, 2, 13, 11, 64),
                                           (3, 0, 3, 27, 27, 192), (2, 0, 3, 12, 10, 64)])
def test_fp32_emulation_of_the_pooled_reduce_link(k, pad, N, H, W, C, dtype):
    """The pooled reduce's formula in plain fp32 from the emulated 16-bit ``out`` agrees with the sums over the true y
    at the argmax within the link bound, and with ``out`` of the neighbouring window it fails."""
    d = cc.stem_tail_operands(N, H, W, "real", dtype, C=C, pad=pad, seed=5)
    OH, OW = pc.out_hw(H, W, k, pad)
    dp = d["dp"] if k == 3 else torch.randn(N, OH, OW, C, generator=torch.Generator().manual_seed(5)).to(dtype)
    out, idx = pc.pool_fwd_emul(d["y"], d["coef"], dtype, k, pad, 255 if k == 3 else None)
    ref, mag, carry = pc.pooled_link_ref(d["y"], d["coef"], dp, idx, out, k, pad, dtype)
    n_chain = pc.reduce16_plan(N * OH * OW, C, 2048)[2]

    def formula(o):
        c = d["coef"]
        of = o.float()
        dz = torch.where(of > 0, dp.float(), torch.zeros(()))
        xh = ((of - c[C:2 * C]) * (1.0 / c[:C]) - c[2 * C:3 * C]) * c[3 * C:4 * C]
        return torch.stack([dz.reshape(-1, C).sum(0), (dz * xh).reshape(-1, C).sum(0)], 1).double()

    pc.assert_pooled_link(formula(out), ref, mag, carry, n_chain, "emulation")
    with pytest.raises(AssertionError):
        pc.assert_pooled_link(formula(out.roll(1, 2)), ref, mag, carry, n_chain, "neighbouring window")


# ------------------------------------------------------------------------------------------------ vgg.hip
POOL2_SHAPES = [(3, 12, 10, 64), (2, 2, 2, 8), (1, 6, 4, 8), (2, 4, 6, 512), (5, 14, 14, 24)]


def _pool2_bwd_emul(d, idx, out, dtype):
    """Plain fp32 evaluation of maxpool2_bwd, rounded once to ``dtype``."""
    N, H, W, C = d["y"].shape
    g = torch.where(out.float() > 0, d["dp"].float(), torch.zeros(()))
    dz = torch.zeros(N, H, W, C)
    for k in range(4):
        dz[:, k >> 1::2, k & 1::2] = torch.where(idx == k, g, torch.zeros(()))
    if d["b"] is None:
        return dz.to(dtype)
    b = d["b"]
    return (b[:C] * dz + b[C:2 * C] * d["y"].float() + b[2 * C:3 * C]).to(dtype)


@pytest.mark.parametrize("dtype", cc.DTYPES)
@pytest.mark.parametrize("form,layer", [("bn", "real"), ("bn", "int"), ("bias", "real")])
@pytest.mark.parametrize("N,H,W,C", POOL2_SHAPES)
def test_fp32_emulation_of_the_2x2_pool_and_its_backward(N, H, W, C, form, layer, dtype):
    """The emulation passes the forward rules on the raw operands and, after ``make_decisive`` (no undecisive window is
    left: checked from the reference alone), the backward bound; the integer layer is exactly representable and fully
    pinned; one ulp16, a dropped window member, an argmax shifted by one and coefficients shifted by one channel fail."""
    exact = layer == "int"
    d = pc.pool2_operands(N, H, W, C, layer, dtype, form)
    r = pc.pool_fwd_ref(d["y"], d["coef"], 2, 0)
    out, idx = pc.pool_fwd_emul(d["y"], d["coef"], dtype, 2, 0, None)
    pc.assert_pool_fwd(out, idx, r, dtype, None, "emulation", exact=exact)
    d["y"] = pc.make_decisive(d["y"], d["coef"], dtype, 2, 0, seed=H * W + C)
    r = pc.pool_fwd_ref(d["y"], d["coef"], 2, 0)
    assert bool(pc.settled(r).all())
    out, idx = pc.pool_fwd_emul(d["y"], d["coef"], dtype, 2, 0, None)
    pc.assert_pool_fwd(out, idx, r, dtype, None, "emulation", exact=exact)
    assert torch.equal(idx.long(), r["first"]) and torch.equal(out.double() > 0, r["ref"] > 0)
    dz, ref, mag = pc.pool2_bwd_ref(d, r)
    if exact:
        assert bool((r["decisive"] | r["must_dead"]).all())
        for v in (r["ref"], ref):
            assert bool((nm.round_exact(v, dtype) == v).all())

    def judge(dy):
        if form == "bias":
            nm.assert_exact(dy, dz, "dy")
        elif exact:
            nm.assert_exact(dy, nm.round_exact(ref, dtype), "dy")
        else:
            nm.assert_rounded(dy, ref, mag, dtype, name="dy", C=C)

    judge(_pool2_bwd_emul(d, idx, out, dtype))
    # forward mutations
    bad = _bump(out, r["ref"], None, exact)
    if bad is not None:
        with pytest.raises(AssertionError, match="out"):
            pc.assert_pool_fwd(bad, idx, r, dtype, None, "one ulp", exact=exact)
    drop = r["win"].clone()
    drop.scatter_(-1, r["first"].unsqueeze(-1), -1.0)
    if bool((drop.max(-1).values.clamp_min(0) != r["ref"]).any()):
        with pytest.raises(AssertionError, match="out"):
            pc.assert_pool_fwd(drop.max(-1).values.clamp_min(0).to(dtype), idx, r, dtype, None, "dropped member",
                               exact=exact)
    at = tuple(r["decisive"].nonzero()[0].tolist())
    shifted = idx.clone()
    shifted[at] = (int(idx[at]) + 1) % 4
    with pytest.raises(AssertionError):
        pc.assert_pool_fwd(out, shifted, r, dtype, None, "argmax + 1", exact=exact)
    if form == "bn":
        rolled = torch.cat([d["coef"][:C].roll(1), d["coef"][C:2 * C].roll(1), d["coef"][2 * C:]])
        o2, i2 = pc.pool_fwd_emul(d["y"], rolled, dtype, 2, 0, None)
        with pytest.raises(AssertionError):
            pc.assert_pool_fwd(o2, i2, r, dtype, None, "channel + 1", exact=exact)
    # backward mutations: an argmax shifted by one in every window; coefficients of the neighbouring channel; one ulp
    with pytest.raises(AssertionError):
        judge(_pool2_bwd_emul(d, (idx + 1) % 4, out, dtype))
    if form == "bn":
        with pytest.raises(AssertionError):
            judge(_pool2_bwd_emul(dict(d, b=d["b"].view(3, C).roll(1, 1).reshape(-1)), idx, out, dtype))
        with pytest.raises(AssertionError):
            judge(_bump(_pool2_bwd_emul(d, idx, out, dtype), ref, None, exact))


def test_vgg_hash_forms_agree_and_match_hand_checked_values():
    """vgg_hash is the splitmix64 output function of seed + 0x9E3779B97F4A7C15 * (i + 1), upper 32 bits.  With seed 0
    the elements 0, 1, 2 are the first three outputs of splitmix64 seeded with 0 -- 0xE220A8397B1DCDAF,
    0x6E789E6AA1B965F4, 0x06C45D188009454F, the published test vector -- whose upper halves are checked here; the
    first was also followed by hand: z0 = 0x9E3779B97F4A7C15, z0 ^ (z0 >> 30) = 0x9E3779BB07979AF0."""
    z0 = 0x9E3779B97F4A7C15
    assert z0 ^ (z0 >> 30) == 0x9E3779BB07979AF0
    assert [pc.vgg_hash_int(0, i) for i in range(3)] == [0xE220A839, 0x6E789E6A, 0x06C45D18]
    assert list(pc.vgg_hash_np(0, 3)) == [0xE220A839, 0x6E789E6A, 0x06C45D18]
    for seed in (0, 11, 2 ** 63 - 1):
        for start in (0, 2 ** 27 + 5):
            want = [pc.vgg_hash_int(seed, start + i) for i in range(64)]
            assert list(pc.vgg_hash_np(seed, 64, start)) == want
            assert pc.vgg_hash_torch(seed, 64, start, "cpu").tolist() == want
    assert pc.dropout_consts(2.0 ** -33) == (1, 1.0) and pc.dropout_consts(0.5) == (2 ** 31, 2.0)
    assert pc.dropout_consts(0.0) == (0, 1.0) and pc.dropout_consts(0.999)[0] == int(0.999 * 2 ** 32)


@pytest.mark.parametrize("dtype", cc.DTYPES)
def test_fc_act_reference_is_the_fp32_evaluation_and_rejects_a_shifted_keep_mask(dtype):
    g = torch.Generator().manual_seed(5)
    rows, F_, p, seed = 37, 136, 0.1, 11
    z, bias = torch.randn(rows, F_, generator=g).to(dtype), torch.randn(F_, generator=g) * 0.5
    thr, scale = pc.dropout_consts(p)
    keep = torch.from_numpy(pc.vgg_hash_np(seed, rows * F_) >= thr).view(rows, F_)
    emul = torch.where(keep, torch.relu(z.float() + bias) * scale, torch.zeros(())).to(dtype)
    nm.assert_exact(emul, pc.fc_act_ref(z, bias, F_, p, keep, dtype), "fc_act_fwd emulation")
    with pytest.raises(AssertionError):
        nm.assert_exact(emul, pc.fc_act_ref(z, bias, F_, p, keep.roll(1, 1), dtype), "keep mask + 1")
    with pytest.raises(AssertionError):
        nm.assert_exact(emul, pc.fc_act_ref(z, bias.roll(1), F_, p, keep, dtype), "bias + 1")
    dh = torch.randn(rows, F_, generator=g).to(dtype)
    dz = torch.where(emul > 0, dh.float() * scale, torch.zeros(())).to(dtype)
    nm.assert_exact(dz, pc.fc_act_bwd_ref(dh, emul, p, dtype), "fc_act_bwd emulation")
    with pytest.raises(AssertionError):
        nm.assert_exact(dz, pc.fc_act_bwd_ref(dh, emul, 0.0, dtype), "scale dropped")


@pytest.mark.parametrize("dtype", cc.DTYPES)
@pytest.mark.parametrize("layer", ["int", "real"])
@pytest.mark.parametrize("case", cc.FIRST_CONV)
def test_first_conv_window_maps_and_weight_gradient_assertion(case, layer, dtype):
    """The production index maps of the first conv (executor_vgg.first_conv_maps): the forward map lays every weight at
    window (r, s // 8), element (s % 8) * 4 + c and zero elsewhere; the gradient map reads it back.  A plain fp32
    weight gradient laid out as the kernel's window tile (padding row and columns filled with finite garbage) and gathered
    through the map passes the bound (``int``: exact, every sum below 2**24); a dropped kernel row does not."""
    from pytorch_distributed_template_amd.models.executor_vgg import first_conv_maps
    R, st, pad, N, H, W = case
    x, wk, dy = cc.first_conv_operands(case, dtype, layer)
    win, gidx, T, U, ldw = first_conv_maps(64, R)
    assert (T, U, ldw) == ((R + 1) // 2, (R + 7) // 8, (R + 1) // 2 * ((R + 7) // 8) * 64)
    flat = wk.reshape(-1)
    wwin = torch.where(win >= 0, flat[win.clamp_min(0).long()], torch.zeros((), dtype=dtype)).view(64, R, U, 8, 4)
    expect = torch.zeros(64, R, U * 8, 4, dtype=dtype)
    expect[:, :, :R, :3] = wk
    assert torch.equal(wwin.reshape(64, R, U * 8, 4), expect)
    xr = x.to(dtype).permute(0, 2, 3, 1).contiguous()
    ref, mag = nm.conv_wgrad_ref(xr, dy, R, R, st, pad)
    if layer == "int":
        assert float(mag.max()) < 2.0 ** 24
    dw = torch.nn.grad.conv2d_weight(xr.float().permute(0, 3, 1, 2), (64, 3, R, R), dy.float().permute(0, 3, 1, 2),
                                     stride=st, padding=pad).permute(0, 2, 3, 1).contiguous()  # KRSC, plain fp32
    tile = torch.full((64, T, U, 2, 8, 4), 7.5)
    for r in range(R):
        for s in range(R):
            tile[:, r // 2, s // 8, r % 2, s % 8, :3] = dw[:, r, s]
    n = N * ((H + 2 * pad - R) // st + 1) * ((W + 2 * pad - R) // st + 1)

    def judge(t):
        got = t.reshape(-1)[gidx.long()].view(64, R, R, 3)
        if layer == "int":
            nm.assert_exact(got, ref.float().double(), "dw")
        else:
            nm.assert_conv(got, ref, mag, n, torch.float32, "dw", None)

    judge(tile)
    dropped = tile.clone()
    dropped[:, (R - 1) // 2, :, (R - 1) % 2] = 0  # the last kernel row
    with pytest.raises(AssertionError):
        judge(dropped)


@pytest.mark.parametrize("dtype", cc.DTYPES)
@pytest.mark.parametrize("nhw", [(2, 29, 28), (2, 8, 32)])
def test_fp32_emulation_of_the_16_bit_fused_stem_weight_gradient(nhw, dtype):
    """dY in plain fp32, rounded to the dtype, then a plain fp32 conv2d_weight: inside nm.stem_fused_bound; the argmax
    of ``cc.stem_fused_operands`` is consistent with y (no routed gradient meets a non-positive pre-activation); dY of
    the neighbouring channel's coefficients is outside.  The integer layer's dY is representable and its sums exact."""
    N, H, W = nhw
    P, Q = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    for layer in ("int", "real"):
        d = cc.stem_fused_operands(N, H, W, dtype, layer)
        r = cc.stem_tail_ref(d, N, P, Q, 64)
        assert float((r["dzraw"] - r["dz"]).abs().max()) == 0.0
        xr = d["x"].to(dtype).permute(0, 2, 3, 1).contiguous()
        ref, mag = nm.conv_wgrad_ref(xr, r["dy"], 7, 7, 2, 3)

        def emul(b):
            dy = (b[:64] * r["dzraw"].float() + b[64:128] * d["y"].float() + b[128:192]).to(dtype)
            return torch.nn.grad.conv2d_weight(xr.float().permute(0, 3, 1, 2), (64, 3, 7, 7), dy.float().permute(0, 3, 1, 2),
                                               stride=2, padding=3).permute(0, 2, 3, 1)
        if layer == "int":
            assert bool((nm.round_exact(r["dy"], dtype) == r["dy"]).all()) and 2 * float(mag.max()) < 2.0 ** 24
            nm.assert_exact(emul(d["b"]), ref.float().double(), "emulation")
            continue
        bound = nm.stem_fused_bound(xr, r["dy"], r["dymag"], N * P * Q, dtype)
        nm.assert_within(emul(d["b"]), ref, bound, "emulation", 3, f"cpu_plain_conv16_stem_fused/{str(dtype).split('.')[-1]}")
        with pytest.raises(AssertionError):
            nm.assert_within(emul(d["b"].view(3, 64).roll(1, 1).reshape(-1)), ref, bound, "channel + 1", 3)
