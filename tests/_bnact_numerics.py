"""fp64 references and derived bounds of the fused BatchNorm + activation kernels (csrc/kernels/bnact.hip); a plain
module shared by tests/test_bnact_cpu.py and tests/test_bnact_gpu.py, on top of tests/_numerics.py (u = 2**-24).

Notation: ``u = x*scale + shift`` (fp32, one fused multiply-add in the kernels), ``mag_u = |x*scale| + |shift|``,
``act'`` with torch's breakpoint conventions (relu' = [u > 0], relu6' = [0 < u < 6], hardswish' = 0 for u <= -3,
(2u + 3)/6 for -3 < u < 3, 1 from 3 on: aten's hardswish_backward).

* bnact_fwd: ``half_ulp16 + 8u * mag``.  identity / relu / relu6 are 1-Lipschitz and add no rounding: mag = mag_u (u is
  rounded at most twice).  hardswish = u * t / 6 with t = clamp(u + 3, 0, 6): with du <= 2u*mag_u, dt <= du +
  u(|u| + 3), the product and the division each one more rounding, the error is at most
  2u * [mag_u(|t| + |u|)/6 + |u|(|u| + 3)/6 + |out|]; mag is that bracket.
* dz = g * act'(u).  For the piecewise-constant act' it is g or 0 exactly: |dz| magnitude |g| * |act'|.  For hardswish's
  middle branch act' = (2u + 3)/6 inherits du/3 <= 2u*mag_u/3 and is rounded twice (sum, division), g * act' once
  more: the error of dz is at most u|g|(2 mag_u/3 + 3|act'|) and of dz * xhat (two roundings in xhat, one product)
  u|g||xhat|(2 mag_u/3 + 6|act'|) = 4u * |g| * M * |xhat| with **M = 1.5|act'| + mag_u/6**, the activation-gradient
  magnitude used below (M = |act'| elsewhere, where at most 3 roundings touch a term).
* bnact_bwd_reduce: ``(n_chain + 4)u * sum|term|`` with |term| = |g| M and |g| M |xhat|, n_chain = ceil(rows / (blocks *
  lanes)) + lanes (a thread's chain, then the fp32 sum over the block's row lanes; fp64 afterwards).
* bnact_bwd_apply: ``half_ulp16 + 8u * mag``, mag = |A| |g| M + |B x| + |Cc| (dz: at most 4, the two fused
  multiply-adds 2 more).
* A reference u closer to a breakpoint than ``8u * mag_u`` could legitimately take the other branch in fp32
  (``near_breakpoint``); the tests choose seeds where no element does and assert that count is 0.
"""
import torch

import _numerics as nm
from _numerics import U

ACTS = ("identity", "relu", "relu6", "hardswish")
BREAKPOINTS = {"identity": (), "relu": (0.0,), "relu6": (0.0, 6.0), "hardswish": (-3.0, 3.0)}


def u_ref(x, coef, C):
    """fp64 (u, mag_u) from the 16-bit x and the fp32 [scale | shift | ...] the kernel reads."""
    x64, c = x.to(torch.float64).reshape(-1, C), coef.to(torch.float64)
    t1, t2 = x64 * c[:C], c[C:2 * C]
    return t1 + t2, t1.abs() + t2.abs()


def act_ref(u, act):
    if act == "relu":
        return u.clamp_min(0.0)
    if act == "relu6":
        return u.clamp(0.0, 6.0)
    if act == "hardswish":
        return u * (u + 3.0).clamp(0.0, 6.0) / 6.0
    return u


def dact_ref(u, act):
    one, zero = torch.ones_like(u), torch.zeros_like(u)
    if act == "relu":
        return torch.where(u > 0, one, zero)
    if act == "relu6":
        return torch.where((u > 0) & (u < 6), one, zero)
    if act == "hardswish":
        return torch.where(u <= -3, zero, torch.where(u < 3, (2.0 * u + 3.0) / 6.0, one))
    return one


def dact_mag(u, mag_u, act):
    d = dact_ref(u, act).abs()
    if act == "hardswish":
        return torch.where((u > -3) & (u < 3), 1.5 * d + mag_u / 6.0, d)
    return d


def near_breakpoint(u, mag_u, act):
    """Elements whose reference u lies within 8u * mag_u of a breakpoint of ``act``."""
    near = torch.zeros_like(u, dtype=torch.bool)
    for b in BREAKPOINTS[act]:
        near |= (u - b).abs() <= 8 * U * mag_u
    return near


def fwd_ref(x, coef, C, act):
    """(u, mag_u, out, mag) of bnact_fwd."""
    u, mag_u = u_ref(x, coef, C)
    out = act_ref(u, act)
    if act == "hardswish":
        t = (u + 3.0).clamp(0.0, 6.0)
        mag = mag_u * (t.abs() + u.abs()) / 6.0 + u.abs() * (u.abs() + 3.0) / 6.0 + out.abs()
    else:
        mag = mag_u
    return u, mag_u, out, mag


def dz_ref(g, x, coef, C, act):
    """(dz, |g| M) in fp64."""
    u, mag_u = u_ref(x, coef, C)
    g64 = g.to(torch.float64).reshape(-1, C)
    return g64 * dact_ref(u, act), g64.abs() * dact_mag(u, mag_u, act)


def bwd_reduce_ref(g, x, coef, C, act):
    """fp64 ([C, 2] sums, [C, 2] sums of |term|): sum dz, sum dz * xhat with xhat from the fp32 mean / invstd."""
    dz, dzm = dz_ref(g, x, coef, C, act)
    c = coef.to(torch.float64)
    xh = (x.to(torch.float64).reshape(-1, C) - c[2 * C:3 * C]) * c[3 * C:4 * C]
    return (torch.stack([dz.sum(0), (dz * xh).sum(0)], 1), torch.stack([dzm.sum(0), (dzm * xh.abs()).sum(0)], 1))


def bwd_apply_ref(g, x, coef, bcoef, C, act):
    """fp64 (dx, mag) of bnact_bwd_apply."""
    dz, dzm = dz_ref(g, x, coef, C, act)
    b = bcoef.to(torch.float64)
    t2, t3 = b[C:2 * C] * x.to(torch.float64).reshape(-1, C), b[2 * C:3 * C]
    return b[:C] * dz + t2 + t3, b[:C].abs() * dzm + t2.abs() + t3.abs().expand_as(t2)


def n_chain(rows, blocks, lanes):
    return -(-rows // (blocks * lanes)) + lanes


# ------------------------------------------------------------------------------ plain fp32 evaluation (what a correct
# kernel computes before rounding to 16 bits); u is one fused multiply-add: the exact fp64 value rounded once
def u_emul(x, coef, C):
    return (x.to(torch.float64).reshape(-1, C) * coef[:C].double() + coef[C:2 * C].double()).float()


def act_emul(u, act):
    if act == "relu":
        return torch.where(u <= 0, torch.zeros_like(u), u)
    if act == "relu6":
        return u.clamp(0.0, 6.0)
    if act == "hardswish":
        return u * (u + 3.0).clamp(0.0, 6.0) / 6.0
    return u


def dz_emul(g, u, act):
    g = g.float().reshape(u.shape)
    zero = torch.zeros_like(g)
    if act == "relu":
        return torch.where(u > 0, g, zero)
    if act == "relu6":
        return torch.where((u > 0) & (u < 6), g, zero)
    if act == "hardswish":
        return torch.where(u <= -3, zero, torch.where(u < 3, g * ((2.0 * u + 3.0) / 6.0), g))
    return g


def bwd_apply_emul(dz, x, bcoef, C):
    return bcoef[:C] * dz + (bcoef[C:2 * C] * x.float().reshape(-1, C) + bcoef[2 * C:3 * C])


# ------------------------------------------------------------------------------------------------------- assertions
def assert_fwd(out, x, coef, C, act, dtype, name="bnact_fwd", family=None):
    _, _, ref, mag = fwd_ref(x, coef, C, act)
    return nm.assert_rounded(out.reshape(-1, C), ref, mag, dtype, name=name, C=C, family=family)


def assert_bwd_apply(dx, g, x, coef, bcoef, C, act, dtype, name="bnact_bwd_apply", family=None):
    ref, mag = bwd_apply_ref(g, x, coef, bcoef, C, act)
    return nm.assert_rounded(dx.reshape(-1, C), ref, mag, dtype, name=name, C=C, family=family)


def assert_bwd_sums(got, g, x, coef, C, act, chain, name="bnact_bwd_reduce", family=None):
    """``got``: fp64 [C, 2]."""
    ref, mag = bwd_reduce_ref(g, x, coef, C, act)
    return nm.assert_sum(got, ref, mag, chain, name, 2, family=family)
