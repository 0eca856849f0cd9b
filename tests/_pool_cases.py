"""References, bounds and assertions of the 16-bit pooling kernels (pool.hip, vgg.hip), shared by
tests/test_stem_tail_numerics_gpu.py, tests/test_vgg_kernels_gpu.py (the kernels) and tests/test_numerics_model_cpu.py
(the proofs that a plain fp32 evaluation passes every assertion and that each assertion rejects the listed mutations).  A
plain module; everything runs on the device of its operands.

Forward, out = max over the window of relu(y * scale + shift), rounded once to the 16-bit type (u = 2**-24):

* Each window member is one fp32 multiply and add (or one fma) of exactly representable inputs: at most 2 roundings,
  ``|val - ref| <= 2u * mag_k`` with ``mag_k = |y * scale| + |shift|``; the model keeps the elementwise budget
  ``8u * mag_k`` of tests/_numerics.py.  The maximum of values each off by at most ``B = 8u * max_k mag_k`` is off by at
  most B, and the store rounds once: ``|out - ref| <= half_ulp16(ref) + B``.
* The argmax is decided on the fp32 values BEFORE the rounding to 16 bits, so no half_ulp16 enters its rules.  The
  chosen member's fp32 value is >= the fp32 value of the fp64 maximum's member; each is off by at most 2u * mag (a
  quarter of B), so the chosen member's fp64 value is within B of the fp64 maximum.
* A window is *decisive* where its largest distinct fp64 value is more than 2B above the next distinct one: then fp32
  orders them as fp64 does, and idx must name the first scan position (kh * 3 + kw, or dh * 2 + dw) that holds the
  maximum -- members equal in fp64 come from the same y and coefficients, are equal in fp32 too, and the strict
  ``val > best`` keeps the first.
* MaxPool(3, 2): the dead code 255 is REQUIRED where every in-image member has ``pre + 8u * mag <= 0`` (fp32 cannot see
  a positive value) and FORBIDDEN where some member has ``pre - 8u * mag > 0``; in between either is right.
  MaxPool(2, 2) has no dead code: a window of the first kind gives out = 0, idx = 0.

Backward, gather form (maxpool_bwd_relu): a pixel collects at most 4 window gradients in fp32 and rounds once:
``half_ulp16(ref) + (4 + 4) * u * sum|dp|`` (``nm.assert_sum`` with a chain of 4).  Elements whose pre-activation is
within 8u * mag of zero are not compared (the ReLU sign fp32 may call either way); their share is a condition on the
operands (<= 1 %) that tests/test_numerics_model_cpu.py checks from the reference alone.

stem_pool_bwd_apply adds dY = A * dz + B * y + Cc (the 8u elementwise budget) on top of the 4 collected gradients:
``half_ulp16(ref) + 12u * (|A| * sum|dp| + |B * y| + |Cc|)``.

stem_pool_bwd_reduce visits the pooled elements: a thread adds one (masked) gradient per pooled pixel it owns, so with
the lane plan of col_reduce.h (``rpi = 256 // (C / 8)`` row lanes, at least 8 rows per thread, at most 4096 blocks) the
chain is ``ceil(rows / (blocks * rpi)) + rpi`` additions, rows = N * OH * OW; xhat = (y - mean) * invstd and the product
with dz are three more roundings, inside the ``+ 4`` of ``(n_chain + 4) * u * mag``.  A pixel whose ReLU sign is unsure
may contribute its gradients or nothing: ``extra``.

The pooled reduce (stem_pool_bwd_reduce_out / pooled_bwd_reduce) recovers the BN input from the stored 16-bit maximum:
``a = (out - shift) / scale``.  Against the sums over the TRUE y at the argmax its bound is the formula bound of
tests/test_col_reduce_gpu.py, ``(n_chain + 8) * u * sum|dz| * invstd * (|a| + |mean|)``, plus the rounding of out carried
into xhat: ``sum |dz| * half_ulp16(out) * |1 / scale| * invstd``.  An element whose fp64 pre-activation is within
``half_ulp16(pre) + 8u * mag`` of zero may be masked either way (``extra``).
"""
import math

import torch
import torch.nn.functional as F

import _numerics as nm
from _numerics import U


def out_hw(H, W, k, pad):
    return (H + 2 * pad - k) // 2 + 1, (W + 2 * pad - k) // 2 + 1


def windows(v, fill, k, pad):
    """[N, H, W, C] -> [N, OH, OW, C, k*k]: the k x k / stride 2 / ``pad`` windows in scan order, positions outside the
    image = ``fill``."""
    N, H, W, C = v.shape
    OH, OW = out_hw(H, W, k, pad)
    p = F.pad(v.permute(0, 3, 1, 2), (pad, pad, pad, pad), value=fill) if pad else v.permute(0, 3, 1, 2)
    cols = F.unfold(p.contiguous(), (k, k), stride=2).view(N, C, k * k, -1)[..., :OH * OW].view(N, C, k * k, OH, OW)
    return cols.permute(0, 3, 4, 1, 2).contiguous()


def pool_fwd_ref(y, coef, k, pad):
    """fp64 reference of bn_relu_maxpool (k = 3) / bn_relu_maxpool2 (k = 2) from the 16-bit y and the fp32 coefficients
    the kernel reads.  Returns dict: win (relu values per member, -1 outside the image), ref (window maximum), B
    (8u * largest member mag), first (first scan position holding the maximum), decisive, must_dead, must_live."""
    C = y.shape[-1]
    c64 = coef.to(torch.float64)
    t1, t2 = y.to(torch.float64) * c64[:C], c64[C:2 * C]
    pre, mag = t1 + t2, t1.abs() + t2.abs().expand_as(t1)
    inside = windows(torch.ones_like(pre), 0.0, k, pad) > 0
    prew, bw = windows(pre, 0.0, k, pad), 8 * U * windows(mag, 0.0, k, pad)
    win = torch.where(inside, prew.clamp_min(0.0), torch.full_like(prew, -1.0))
    ref = win.max(-1).values
    B = bw.max(-1).values
    pos = torch.arange(k * k, device=y.device)
    first = torch.where(win == ref.unsqueeze(-1), pos, k * k).min(-1).values
    second = torch.where(win < ref.unsqueeze(-1), win, torch.full_like(win, -1.0)).max(-1).values
    return dict(win=win, ref=ref, B=B, first=first, decisive=(ref - second.clamp_min(0.0) > 2 * B) & (ref > 2 * B),
                must_dead=((prew + bw <= 0) | ~inside).all(-1), must_live=((prew - bw > 0) & inside).any(-1), k=k)


def pool_fwd_emul(y, coef, dtype, k, pad, dead_code):
    """What a correct kernel computes: fp32 multiply and add, the first fp32 maximum, one rounding to ``dtype``."""
    C = y.shape[-1]
    val = torch.relu(y.float() * coef[:C] + coef[C:2 * C])
    win = windows(val, -1.0, k, pad)
    best = win.max(-1).values
    pos = torch.arange(k * k)
    idx = torch.where(win == best.unsqueeze(-1), pos, k * k).min(-1).values
    if dead_code is not None:
        idx = torch.where(best > 0, idx, torch.full_like(idx, dead_code))
    return best.to(dtype), idx.to(torch.uint8)


def _first_bad(mask):
    bad = mask.nonzero()
    return int(bad.shape[0]), (tuple(bad[0].tolist()) if bad.shape[0] else None)


def assert_pool_fwd(out, idx, r, dtype, dead_code, name, family=None, exact=False):
    """``out`` [N, OH, OW, C] and ``idx`` (or None: the eval form) against ``pool_fwd_ref``'s ``r`` by the rules of the
    module docstring; ``exact``: a zero bound on ``out`` (the integer layer).  Returns the worst error / bound ratio."""
    ref, B, k = r["ref"], r["B"], r["k"]
    C = ref.shape[-1]
    if exact:
        worst = nm.assert_exact(out, nm.round_exact(ref, dtype), f"{name}: out")
    else:
        worst = nm.assert_within(out, ref, nm.half_ulp16(ref, dtype) + B, f"{name}: out", C, family, ref.shape)
    if idx is None:
        return worst
    i64 = idx.long()
    if dead_code is not None:
        dead = i64 == dead_code
        n, at = _first_bad(dead & r["must_live"])
        assert n == 0, f"{name}: {n} windows with a surely positive member carry the dead code; first at {at}"
        n, at = _first_bad(~dead & r["must_dead"])
        assert n == 0, f"{name}: {n} windows without a positive member carry no dead code; first at {at}: {int(idx[at]) if at else ''}"
    else:
        dead = torch.zeros_like(i64, dtype=torch.bool)
        n, at = _first_bad((i64 != 0) & r["must_dead"])
        assert n == 0, f"{name}: {n} all-dead windows with idx != 0; first at {at}"
    live = ~dead
    n, at = _first_bad(live & (i64 >= k * k))
    assert n == 0, f"{name}: {n} argmax bytes unwritten or no window position; first at {at}"
    chosen = r["win"].gather(-1, i64.clamp_max(k * k - 1).unsqueeze(-1)).squeeze(-1)
    n, at = _first_bad(live & (chosen < 0))
    assert n == 0, f"{name}: {n} argmax bytes name a position outside the image; first at {at}"
    nm.assert_within(chosen[live], ref[live], B[live], f"{name}: value at idx", None, family)
    n, at = _first_bad(live & r["decisive"] & (i64 != r["first"]))
    assert n == 0, (f"{name}: {n} decisive windows with another argmax; first at {at}: got {int(idx[at]) if at else ''}, "
                    f"expected {int(r['first'][at]) if at else ''}")
    return worst


def decisive_planes(N, H, W, C, seed):
    """The integer ``decisive`` operands of test_bn_relu_maxpool32_decisive as fp32 CPU tensors (y, coef): a per-plane
    permutation of -4 .. 4 laid out by (h % 3, w % 3) -- the 9 values of every 3x3 window differ --, planes c % 8 == 5
    hold -9 .. -1 under a positive scale (all-negative windows), power-of-two scales of mixed sign, shift 0.5."""
    g = torch.Generator().manual_seed(seed)
    perm = (torch.argsort(torch.rand(N, C, 9, generator=g), dim=-1) - 4).float()
    ch = torch.arange(C)
    perm[:, ch % 8 == 5] -= 5.0
    pos = (torch.arange(H).view(H, 1) % 3) * 3 + torch.arange(W).view(1, W) % 3
    y = perm[:, :, pos].permute(0, 2, 3, 1).contiguous()
    scale = torch.tensor([1.0, 2.0, 4.0])[ch % 3] * torch.where((ch // 3) % 2 == 0, 1.0, -1.0)
    scale[ch % 8 == 5] = 2.0
    return y, torch.cat([scale, torch.full((C,), 0.5), torch.zeros(2 * C)]).contiguous()


# ------------------------------------------------------------------------------------------------ backward
def assert_pool_bwd(dz, r, dtype, name, family=None, exact=False):
    """maxpool_bwd_relu's dz against ``cc.stem_tail_ref``'s ``r``: chain of 4 plus the rounding, unsure elements left
    out.  Returns (worst ratio, compared share)."""
    sure = ~r["unsure"]
    share = float(sure.double().mean().item())
    assert bool(torch.isfinite(dz.float()).all()), f"{name}: an element was not written"
    if exact:
        return nm.assert_exact(dz, nm.round_exact(r["dz"], dtype), name), share
    bound = nm.half_ulp16(r["dz"], dtype) + (4 + 4) * U * r["dzmag"]
    return nm.assert_within(dz[sure], r["dz"][sure], bound[sure], name, None, family), share


def assert_tail_apply(dy, r, dtype, name, family=None, exact=False):
    """stem_pool_bwd_apply's dY against ``cc.stem_tail_ref``'s ``r``: half_ulp16(ref) + 12u * dymag, unsure elements left
    out.  Returns (worst ratio, compared share)."""
    sure = ~r["unsure"]
    share = float(sure.double().mean().item())
    assert bool(torch.isfinite(dy.float()).all()), f"{name}: an element was not written"
    if exact:
        return nm.assert_exact(dy, nm.round_exact(r["dy"], dtype), name), share
    bound = nm.half_ulp16(r["dy"], dtype) + 12 * U * r["dymag"]
    return nm.assert_within(dy[sure], r["dy"][sure], bound[sure], name, None, family), share


def reduce16_plan(rows, C, cap):
    """(blocks, rpi, n_chain) of col_plan(rows, C, 8, 2, 8, cap): the 16-bit pooled reduces' lane plan."""
    rpi = 256 // (C // 8)
    blocks = max(1, min(cap, -(-rows // (rpi * 8))))
    return blocks, rpi, math.ceil(rows / (blocks * rpi)) + rpi


def assert_tail_reduce(got, d, r, C, n_chain, name, family=None, exact=False):
    """[C, 2] (sum dz, sum dz * xhat) of stem_pool_bwd_reduce against the independent fp64 dz of ``r``."""
    xh = nm.bn_xhat(d["y"], d["coef"], C)
    dz, dzmag = r["dz"].reshape(-1, C), r["dzmag"].reshape(-1, C)
    ref = torch.stack([dz.sum(0), (dz * xh).sum(0)], 1)
    if exact:
        return nm.assert_within(got, ref, 0.0, name, 2)
    flip = torch.where(r["unsure"].reshape(-1, C), dzmag, torch.zeros_like(dzmag))
    mag = torch.stack([dzmag.sum(0), (dzmag * xh.abs()).sum(0)], 1)
    extra = torch.stack([flip.sum(0), (flip * xh.abs()).sum(0)], 1)
    return nm.assert_within(got, ref, (n_chain + 4) * U * mag + extra, name, 2, family)


def pooled_link_ref(y, coef, dp, idx, out, k, pad, dtype):
    """Reference and bound of the pooled reduce against the TRUE y at the argmax ``idx`` (bytes >= k*k: dead): returns
    (ref [C, 2], mag [C, 2] of the formula bound, carry [C, 2]: the rounding of out carried into xhat plus the elements
    whose mask may go either way)."""
    C = y.shape[-1]
    c64 = coef.to(torch.float64)
    scale, shift, mean, invstd = c64[:C], c64[C:2 * C], c64[2 * C:3 * C], c64[3 * C:4 * C]
    live = idx.long() < k * k
    yw = windows(y.to(torch.float64), 0.0, k, pad)
    ya = yw.gather(-1, idx.long().clamp_max(k * k - 1).unsqueeze(-1)).squeeze(-1)
    t1 = ya * scale
    pre, pmag = t1 + shift, t1.abs() + shift.abs()
    unsure = live & (pre.abs() <= nm.half_ulp16(pre, dtype) + 8 * U * pmag)
    g = dp.to(torch.float64)
    dz = torch.where(live & (pre > 0), g, torch.zeros_like(g))
    xh = (ya - mean) * invstd
    o64 = out.to(torch.float64)
    a = (o64 - shift) / scale
    rs = lambda t: t.reshape(-1, C).sum(0)
    ref = torch.stack([rs(dz), rs(dz * xh)], 1)
    mag = torch.stack([rs(dz.abs()), rs(dz.abs() * invstd * (a.abs() + mean.abs()))], 1)
    flip = torch.where(unsure, g.abs(), torch.zeros_like(g))
    carry = torch.stack([rs(flip), rs(flip * xh.abs()) + rs(dz.abs() * nm.half_ulp16(o64, dtype) * invstd / scale.abs())], 1)
    return ref, mag, carry


def assert_pooled_link(got, ref, mag, carry, n_chain, name, family=None):
    b = torch.stack([(n_chain + 4) * U * mag[:, 0], (n_chain + 8) * U * mag[:, 1]], 1) + carry
    return nm.assert_within(got, ref, b, name, 2, family)


# ------------------------------------------------------------------------------------------------ vgg.hip
def pool2_operands(N, H, W, C, layer, dtype, form="bn", seed=0):
    """Operands of bn_relu_maxpool2 / maxpool2_bwd (CPU): dict y [N, H, W, C] and dp [N, H/2, W/2, C] in ``dtype``, coef
    ([scale | shift | mean | invstd]) and b ([A | B | Cc]) as ``cc.stem32_tail_operands`` makes them (mixed-sign scales;
    layer B: channel 1 at 1e-3), or, ``form="bias"``, coef = [1 | bias | 0 | 1] and b = None."""
    import _conv_cases as cc
    d = cc.stem32_tail_operands(N, H, W, layer, C=C, seed=seed + 31)
    gen = torch.Generator().manual_seed(97 + H * W + C + seed)
    if layer == "int":
        dp = nm.conv_int_operands((N, H // 2, W // 2, C), cc.XVALS, 98 + H + seed)
    else:
        dp = torch.randn(N, H // 2, W // 2, C, generator=gen)
        dp[..., 1] *= 1e-3
        d["coef"][1] *= 1e-3
        d["coef"][C + 1] *= 1e-3
    coef, b = d["coef"].contiguous(), d["b"]
    if form == "bias":
        coef = torch.cat([torch.ones(C), torch.randn(C, generator=gen) * 0.3, torch.zeros(C), torch.ones(C)])
        b = None
    return dict(y=d["y"].to(dtype), dp=dp.to(dtype), coef=coef, b=b)


FP16_MIN_NORMAL = 2.0 ** -14


def settled(r):
    """Windows whose forward result leaves the backward no choice: surely dead, or decisive with a maximum that no 16-bit
    rounding takes to zero."""
    return r["must_dead"] | (r["decisive"] & (r["ref"] > FP16_MIN_NORMAL))


def make_decisive(y, coef, dtype, k, pad, seed, rounds=50):
    """``y`` (CPU, ``dtype``) with every window that is not ``settled`` redrawn (all its members, randn rounded to
    ``dtype``) until none is left: the fp64 argmax and ReLU mask are then what any correct kernel finds."""
    assert k == 2 and pad == 0
    gen = torch.Generator().manual_seed(seed)
    y = y.clone()
    for _ in range(rounds):
        bad = ~settled(pool_fwd_ref(y, coef, k, pad))
        if not bool(bad.any()):
            return y
        full = bad.repeat_interleave(2, 1).repeat_interleave(2, 2)
        y = torch.where(full, torch.randn(y.shape, generator=gen).to(dtype), y)
    raise AssertionError("make_decisive: windows without a decisive argmax are left")


def pool2_bwd_ref(d, r, pos=None, mask=None):
    """fp64 reference of maxpool2_bwd from ``pool_fwd_ref``'s ``r`` (or the given argmax ``pos`` and ReLU ``mask``): dz
    (dp at the window's argmax where the maximum is positive), and for the BN form (dy, mag) of A*dz + B*y + Cc."""
    y, dp = d["y"], d["dp"]
    N, H, W, C = y.shape
    pos = r["first"] if pos is None else pos.long()
    mask = (r["ref"] > 0) if mask is None else mask
    g = torch.where(mask, dp.to(torch.float64), torch.zeros((), dtype=torch.float64, device=y.device))
    dz = torch.zeros(N, H, W, C, dtype=torch.float64, device=y.device)
    for k in range(4):
        dz[:, k >> 1::2, k & 1::2] = torch.where(pos == k, g, torch.zeros_like(g))
    if d["b"] is None:
        return dz, None, None
    dy, mag = nm.bn_bwd_apply_ref(dz, y, d["b"].to(y.device), C)
    return dz, dy.view(N, H, W, C), mag.view(N, H, W, C)


_M64 = (1 << 64) - 1


def vgg_hash_int(seed, i):
    """vgg_hash of vgg.hip in Python integers (the splitmix64 output function of seed + golden * (i + 1), upper 32
    bits)."""
    z = (seed + 0x9E3779B97F4A7C15 * (i + 1)) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return (z ^ (z >> 31)) >> 32


def vgg_hash_np(seed, n, start=0):
    """The same for the elements start .. start + n - 1 in numpy uint64 (wrapping arithmetic): uint32 array."""
    import numpy as np
    with np.errstate(over="ignore"):
        i = np.arange(start + 1, start + n + 1, dtype=np.uint64)
        z = np.uint64(seed) + np.uint64(0x9E3779B97F4A7C15) * i
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return ((z ^ (z >> np.uint64(31))) >> np.uint64(32)).astype(np.uint32)


def _i64(v):
    v &= _M64
    return v - (1 << 64) if v >= (1 << 63) else v


def vgg_hash_torch(seed, n, start, device):
    """The same in torch int64 (two's-complement wrapping products, logical shifts by masking), for references computed on
    the GPU: int64 tensor of values 0 .. 2**32 - 1.  tests/test_numerics_model_cpu.py holds it equal to the numpy form."""
    lsr = lambda z, s: (z >> s) & ((1 << (64 - s)) - 1)
    i = torch.arange(start + 1, start + n + 1, dtype=torch.int64, device=device)
    z = i * _i64(0x9E3779B97F4A7C15) + _i64(seed)
    z = (z ^ lsr(z, 30)) * _i64(0xBF58476D1CE4E5B9)
    z = (z ^ lsr(z, 27)) * _i64(0x94D049BB133111EB)
    return lsr(z ^ lsr(z, 31), 32)


def dropout_consts(p):
    """(keep threshold, fp32 scale) as fc_act_fwd_launch derives them from the double ``p``."""
    if p <= 0.0:
        return 0, 1.0
    t = p * 4294967296.0
    thr = 0xffffffff if t >= 4294967295.0 else int(t)
    return max(thr, 1), float(torch.tensor(1.0 / (1.0 - p), dtype=torch.float32).item())


def fc_act_ref(z, bias, F_, p, keep, dtype):
    """Exact expected output of fc_act_fwd: fl32(z + b) (the correctly rounded fp32 sum: fp64 holds the exact one),
    ReLU, times the fp32 scale where kept (a 48-bit product, exact in fp64), rounded once to fp32 and once to ``dtype``."""
    s32 = (z.to(torch.float64).view(-1, F_) + bias.to(torch.float64)).to(torch.float32).clamp_min(0.0)
    _, scale = dropout_consts(p)
    v = s32.to(torch.float64) * scale
    if keep is not None:
        v = torch.where(keep.view(-1, F_), v, torch.zeros_like(v))
    return nm.round_exact(v, dtype)


def fc_act_bwd_ref(dh, out, p, dtype):
    _, scale = dropout_consts(p)
    return nm.round_exact(torch.where(out.to(torch.float64) > 0, dh.to(torch.float64) * scale,
                                      torch.zeros((), dtype=torch.float64, device=dh.device)), dtype)
