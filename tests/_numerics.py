"""Shared per-element error model of the kernel tests (a plain module, not a conftest).

Every tolerance is derived from the arithmetic the kernels perform, none is tuned.  With ``u = 2**-24`` (the unit
roundoff of fp32, i.e. one rounded fp32 operation on a value v is off by at most ``u * |v|``):

* A kernel that evaluates an expression of a few fp32 operations (multiply, add, fma) on exactly representable inputs
  produces ``val`` with ``|val - ref| <= k * u * mag`` where ``mag`` is the sum of the absolute values of the
  expression's terms and ``k`` bounds the number of roundings any term passes through (k = 8 covers every elementwise
  kernel here with a margin of about two: the longest expression, ``res * rscale + rshift + y * scale + shift``, rounds
  each term at most 4 times).
* Rounding ``val`` to a 16-bit format adds at most half a 16-bit ulp at ``|val|``: bf16 has 8 significand bits, so
  half an ulp is at most ``|ref| * 2**-8``; fp16 has 11, so ``|ref| * 2**-11``, and never less than half the
  subnormal spacing ``2**-25``.
* A sum of n fp32 terms accumulated along a chain of ``n_chain`` additions is off by at most ``n_chain * u * sum|term|``
  (first order); the products feeding the chain and the final fp32 -> fp64 partial sums add a few more ``u``: the model
  uses ``(n_chain + 4) * u * sum|term|``.

References are fp64 and are computed from the very 16-bit / fp32 values the kernel reads, so no input rounding enters
the bounds.  ``tests/test_numerics_model_cpu.py`` proves that a plain fp32 evaluation of every formula stays inside its
bound and that each assertion rejects a one-ulp error, a dropped row and coefficients shifted by one channel.

Each assertion returns the worst observed error / bound ratio and records it per family in ``RATIOS``; with
``PDT_TEST_RATIOS=<file>`` in the environment the table is written there as JSON when the interpreter exits.
"""
import atexit
import json
import os

import torch

U = 2.0 ** -24

RATIOS = {}


def _dump_ratios():
    path = os.environ.get("PDT_TEST_RATIOS")
    if path and RATIOS:
        with open(path, "w") as f:
            json.dump(RATIOS, f, indent=1, sort_keys=True)


atexit.register(_dump_ratios)


def half_ulp16(ref64: torch.Tensor, dtype) -> torch.Tensor:
    """Upper bound on half a ulp of ``dtype`` at ``|ref|`` (zero for fp32 outputs)."""
    a = ref64.abs()
    if dtype == torch.bfloat16:
        return a * 2.0 ** -8
    if dtype == torch.float16:
        return (a * 2.0 ** -11).clamp_min(2.0 ** -25)
    if dtype == torch.float32:
        return torch.zeros_like(a)
    raise ValueError(f"no error model for {dtype}")


def assert_within(got, ref64, bound64, name="value", C=None, family=None) -> float:
    """|got - ref| <= bound for every element; the message names the worst element, its channel, error and bound."""
    got64 = got.detach().to(torch.float64).reshape(-1)
    ref = ref64.detach().to(torch.float64).reshape(-1)
    bound = bound64.detach().to(torch.float64).expand(ref64.shape).reshape(-1) if torch.is_tensor(bound64) \
        else torch.full_like(ref, float(bound64))
    assert got64.shape == ref.shape == bound.shape, f"{name}: shapes {got64.shape} {ref.shape} {bound.shape}"
    err = (got64 - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)  # err > 0 over a zero bound -> inf
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)  # NaN output
    worst = float(ratio.max().item()) if ratio.numel() else 0.0
    if family is not None:
        RATIOS[family] = max(RATIOS.get(family, 0.0), worst)
    if worst > 1.0:
        i = int(ratio.argmax().item())
        nbad = int((ratio > 1.0).sum().item())
        ch = f", channel {i % C}" if C else ""
        raise AssertionError(
            f"{name}: {nbad} of {ratio.numel()} elements out of bound; worst element {i}{ch}: got {got64[i].item()!r}, "
            f"ref {ref[i].item()!r}, error {err[i].item():.6e}, bound {bound[i].item():.6e} (ratio {worst:.3f})")
    return worst


def assert_rounded(out, ref64, mag64, dtype, k=8, name="value", C=None, family=None) -> float:
    """``out`` is an fp32 expression rounded once to ``dtype``: |out - ref| <= half_ulp16(ref) + k*u*mag per element
    (mag = fp64 sum of the absolute values of the expression's terms; fp32 outputs drop the first term)."""
    return assert_within(out, ref64, half_ulp16(ref64, dtype) + k * U * mag64.abs(), name, C, family)


def assert_sum(got64, ref64, mag64, n_chain, name="sum", C=None, family=None) -> float:
    """``got`` is an fp32 accumulation chain of ``n_chain`` additions followed by fp64 sums:
    |got - ref| <= (n_chain + 4)*u*mag per element (mag = fp64 sum of |term|)."""
    return assert_within(got64, ref64, (n_chain + 4) * U * mag64.abs(), name, C, family)


# ------------------------------------------------------------------------------------------------ reference formulas
def bn_apply_ref(y, coef, res, rcoef, C, resmode, relu):
    """fp64 reference of bn_apply over [rows, C] inputs: returns (pre-activation value, output, mag)."""
    y64 = y.to(torch.float64).view(-1, C)
    c64 = coef.to(torch.float64)
    t1, t2 = y64 * c64[:C], c64[C:2 * C]
    val, mag = t1 + t2, t1.abs() + t2.abs()
    if resmode == 1:
        r64 = res.to(torch.float64).view(-1, C)
        val, mag = val + r64, mag + r64.abs()
    elif resmode == 2:
        r64 = res.to(torch.float64).view(-1, C)
        rc = rcoef.to(torch.float64)
        t3, t4 = r64 * rc[:C], rc[C:2 * C]
        val, mag = val + t3 + t4, mag + t3.abs() + t4.abs()
    return val, (val.clamp_min(0.0) if relu else val), mag


def bn_apply_emul(y, coef, res, rcoef, C, resmode, relu):
    """The same formula in plain fp32 (what a correct kernel computes before rounding to 16 bits)."""
    val = y.float().view(-1, C) * coef[:C] + coef[C:2 * C]
    if resmode == 1:
        val = val + res.float().view(-1, C)
    elif resmode == 2:
        val = val + (res.float().view(-1, C) * rcoef[:C] + rcoef[C:2 * C])
    return torch.relu(val) if relu else val


def bn_bwd_apply_ref(dz64, y, b, C):
    """fp64 dy = A*dz + B*y + Cc with b = [A | B | Cc] fp32: returns (dy, mag)."""
    b64 = b.to(torch.float64)
    t1, t2, t3 = b64[:C] * dz64.view(-1, C), b64[C:2 * C] * y.to(torch.float64).view(-1, C), b64[2 * C:3 * C]
    return t1 + t2 + t3, t1.abs() + t2.abs() + t3.abs().expand_as(t1)


def bn_finalize_ref(sum_x, sum_x2, count, gamma, beta, eps, momentum, rm, rv, var=None):
    """fp64 forward finalize from per-channel fp64 sums: dict of mean, var (clamped at 0), invstd, scale, shift and the
    updated running statistics (unbiased variance for count > 1).  ``var``: the biased variance computed by the caller
    (e.g. two-pass ``x.var``) instead of the one-pass ``sum_x2 / count - mean**2``."""
    mean = sum_x / count
    if var is None:
        var = (sum_x2 / count - mean * mean).clamp_min(0.0)
    # the kernels take eps as a float argument: the reference uses the same fp32 value
    eps32 = float(torch.tensor(eps, dtype=torch.float32).item())
    invstd = 1.0 / torch.sqrt(var + eps32)
    g, b = gamma.to(torch.float64), beta.to(torch.float64)
    scale = g * invstd
    mom = float(torch.tensor(momentum, dtype=torch.float32).item())
    unbiased = var * count / (count - 1) if count > 1 else var
    rm64, rv64 = rm.to(torch.float64), rv.to(torch.float64)
    return dict(mean=mean, var=var, invstd=invstd, scale=scale, shift=b - mean * scale, beta=b,
                rm_old=(1 - mom) * rm64, rm_new=mom * mean, rv_old=(1 - mom) * rv64, rv_new=mom * unbiased)


def check_finalize(coef, rm, rv, ref, C, name, family=None):
    """Forward finalize bounds: mean 2u|ref| (one fp64 -> fp32 rounding, margin 2); invstd 4u|ref| (one rounding of a
    correctly rounded fp64 value; scale = gamma * invstd adds one fp32 product: <= 2u, margin 2); shift
    6u(|beta| + |mean*scale|) (rounded mean, rounded scale, their product, the subtraction: 4 roundings of the product
    term, 1 of beta); running stats 6u(|old| + |new|) ((1 - m) rounded, two products, one sum, the fp64 -> fp32
    rounding of the new value: <= 4 per term)."""
    w = 0.0
    w = max(w, assert_within(coef[2 * C:3 * C], ref["mean"], 2 * U * ref["mean"].abs(), f"{name}: mean", C, family))
    w = max(w, assert_within(coef[3 * C:4 * C], ref["invstd"], 4 * U * ref["invstd"].abs(), f"{name}: invstd", C, family))
    w = max(w, assert_within(coef[:C], ref["scale"], 4 * U * ref["scale"].abs(), f"{name}: scale", C, family))
    w = max(w, assert_within(coef[C:2 * C], ref["shift"],
                             6 * U * (ref["beta"].abs() + (ref["mean"] * ref["scale"]).abs()), f"{name}: shift", C, family))
    if rm is not None:
        w = max(w, assert_within(rm, ref["rm_old"] + ref["rm_new"], 6 * U * (ref["rm_old"].abs() + ref["rm_new"].abs()),
                                 f"{name}: running_mean", C, family))
        w = max(w, assert_within(rv, ref["rv_old"] + ref["rv_new"], 6 * U * (ref["rv_old"].abs() + ref["rv_new"].abs()),
                                 f"{name}: running_var", C, family))
    return w


def bn_bwd_finalize_ref(sdz, sdzx, count, coef, gamma, gscale, C):
    """fp64 backward finalize from fp64 sums and the fp32 forward coefficients (mean, invstd) the kernel reads."""
    c64 = coef.to(torch.float64)
    mean, invstd = c64[2 * C:3 * C], c64[3 * C:4 * C]
    A = gamma.to(torch.float64) * invstd
    mdz, mdzx = sdz / count, sdzx / count
    t1, t2 = A * mdz, A * invstd * mdzx * mean
    return dict(dgamma=sdzx * gscale, dbeta=sdz * gscale, A=A, B=-A * invstd * mdzx, Cc=-t1 + t2,
                Cmag=t1.abs() + t2.abs())


def check_bwd_finalize(bcoef, dgamma, dbeta, ref, C, name, family=None):
    """Backward finalize bounds: dgamma / dbeta 2u|ref| (fp64 -> fp32 rounding, one product with gscale); bcoef[0] = A
    4u|ref| (one product, margin for the rounded operands); bcoef[1] = -A*invstd*mdzx 6u|ref| (rounded mdzx, A, two
    products); bcoef[2] 8u(|A*m_dz| + |A*invstd*m_dzx*mean|) (up to 5 roundings of the longer term plus the sum)."""
    w = 0.0
    if dgamma is not None:
        w = max(w, assert_within(dgamma, ref["dgamma"], 2 * U * ref["dgamma"].abs(), f"{name}: dgamma", C, family))
    if dbeta is not None:
        w = max(w, assert_within(dbeta, ref["dbeta"], 2 * U * ref["dbeta"].abs(), f"{name}: dbeta", C, family))
    w = max(w, assert_within(bcoef[:C], ref["A"], 4 * U * ref["A"].abs(), f"{name}: bcoef A", C, family))
    w = max(w, assert_within(bcoef[C:2 * C], ref["B"], 6 * U * ref["B"].abs(), f"{name}: bcoef B", C, family))
    w = max(w, assert_within(bcoef[2 * C:3 * C], ref["Cc"], 8 * U * ref["Cmag"], f"{name}: bcoef C", C, family))
    return w


def sgd_ref(p, g, buf, wd_mask, lr, momentum, wd, gs, steps):
    """fp64 recurrence of the fused SGD over ``steps`` steps with the fp32 hyper-parameters the kernel receives:
    returns (p, buf, bound) with bound = 6u * sum_steps(|p| + lr|buf|) per element (each step rounds d (3 ops), the
    momentum update (2) and the parameter update (2); the error a step inherits is carried by the next step's terms)."""
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float32).item())
    lr, momentum, wd, gs = f32(lr), f32(momentum), f32(wd), f32(gs)
    p64, g64 = p.to(torch.float64).clone(), g.to(torch.float64)
    b64 = buf.to(torch.float64).clone()
    m64 = wd_mask.to(torch.float64) if wd_mask is not None else 1.0
    acc = torch.zeros_like(p64)
    for step in range(steps):
        d = g64 * gs + wd * p64 * m64
        if momentum != 0.0:
            b64 = d if step == 0 else momentum * b64 + d
            b = b64
        else:
            b = d
        acc += p64.abs() + lr * b.abs()
        p64 = p64 - lr * b
    return p64, b64, 6 * U * acc
