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

Convolutions on the MFMA units (16-bit operands, fp32 accumulator), ``U = u = 2**-24``:

* The product of two bf16 values (8 significand bits each) or two fp16 values (11 each) has at most 22 significand
  bits: it is exact in fp32 (fp16 products below 2**-126 do not occur: the smallest non-zero fp16 product is 2**-48).
* Every accumulation into the fp32 accumulator -- one product, a block of products the MFMA has summed internally, a
  split-K partial, a row of ``wgrad_reduce`` -- errs by at most one fp32 ulp of the partial sum it produces, whatever
  rounding mode the unit uses (round-to-nearest would give half of that; the mode for 16-bit inputs is not documented,
  so the model takes the full ulp: ``2u`` relative instead of ``u``).  Every partial sum is bounded in magnitude by
  ``mag``, the same operation applied to the absolute values of the operands.
* A sum of ``n`` terms evaluated in any order and grouping passes through at most ``n - 1`` such accumulations per term
  path, so to first order it is off by at most ``(n - 1) * 2u * mag``; the model uses ``(n + 4) * 2u * mag``, the five
  extra accumulations covering the second-order terms (``n * 2u < 2**-9`` for every n here) and the residual add.
* The 16-bit output rounds the fp32 value once: ``half_ulp16(ref, dtype)`` more.  A residual is added in fp32 before
  that rounding: it is one more term, so ``|residual|`` joins ``mag``.
* Forward and data gradient: ``|out - ref| <= half_ulp16(ref) + (n + 4) * 2u * mag`` with ``n = C*R*S`` (forward) or
  ``Kout * taps of the phase`` (data gradient; ``Kout*R*S`` is a valid upper bound and the one used).
* Weight gradient (fp32 output): ``|dw - ref| <= (n + 4) * 2u * mag``, ``n = N*P*Q``.
* Forward statistics are sums of the ROUNDED outputs (and of their squares, each square one fp32 rounding): they are
  judged with ``assert_sum`` (``n_chain = rows``) against fp64 sums of the stored ``y``; ``y`` itself is held by the
  element bound.
* Fused BN-backward sums are judged against the independent reference ``dz_ref``, never against the kernel's own
  ``dz``: with ``bound_i`` the element bound of ``dz_i``,
  ``|sum dz_k*xhat - sum dz_ref*xhat| <= sum_i bound_i*|xhat_i| + (rows + 4)*u*sum|dz_ref*xhat|`` (the first term is
  the elements' own error carried into the sum, the second the fp32 chain: ``xhat = (y - mean) * invstd`` is two
  roundings, the product one, all inside the ``+ 4`` and the margin of ``rows`` over the real chain length).  The same
  with ``xhat = 1`` for ``sum dz``.  ``xhat`` is taken in fp64 from the fp32 ``mean`` / ``invstd`` the kernel reads.
* Integer operands (``conv_int_operands``): every product and partial sum is an integer far below 2**24, so the fp32
  accumulator is exact in any order; the result is ``ref64`` rounded once to the 16-bit type, bit for bit
  (``assert_exact``: a zero bound).

Convolutions on the fp32 MFMA (v_mfma_f32_16x16x4_f32: fp32 operands, fp32 accumulator; csrc/kernels/fp32.hip):

* The product of two fp32 values has up to 48 significand bits: unlike the 16-bit case it is NOT exact in fp32.  Whether
  the unit rounds each product before adding it or fuses the multiply into the add, a term enters the accumulator with
  at most one rounding of its own: ``2u * |x * w|`` under the same full-ulp convention as above.
* The accumulation is the 16-bit model's: at most ``n - 1`` accumulations per term path, each off by at most one fp32
  ulp of a partial sum bounded by ``mag``; split-K partials and ``wgrad_reduce`` rows are further accumulations of the
  same kind.  Together with the product's rounding a term passes through at most ``n`` roundings:
  ``n * 2u * mag`` to first order.  The model uses ``(n + 5) * 2u * mag``: the 16-bit model's ``n + 4`` plus the one
  rounding per product; the five extra roundings cover the second-order terms (``n * 2u < 2**-10`` up to n = 8192) and
  the residual add.  The output is stored as fp32: no further rounding, no ``half_ulp16`` term.
* Forward and data gradient: ``|out - ref| <= (n + 5) * 2u * mag`` with ``n = C*R*S`` / ``Kout*R*S``; weight gradient
  the same with ``n = N*P*Q`` (``conv32_bound``).  Statistics and fused BN-backward sums are judged exactly as in the
  16-bit case (``assert_conv_stats`` family ``conv32_stats``, ``assert_bnb_sums`` family ``conv32_bnb_sums``).
* Integer operands: every product and partial sum is an integer below 2**24 (checked per case from the reference:
  ``max mag < 2**24`` and every per-channel sum of squares below 2**24), so output, statistics and fused sums EQUAL the
  fp64 reference: there is no representability cap, fp32 holds every such integer.
* The worst-case bound grows with n and says little about the width of the multiply at long reductions (operands rounded
  to 8 bits still pass at n = 4608).  The ``wide`` layer owns that: every output is exactly ONE non-zero product whose
  exact value needs 24 bits, or whose one operand does (``wide_operand``): a product or an operand kept to fewer bits
  changes every element.
* The fused stem weight gradient (``wgrad32_stem_fused``) forms dY = A*dz + B*y + C in the kernel (dz: up to 4 pooled
  gradients added in fp32): each term of dY carries at most 3 + 4 roundings before it meets the product, one more than
  half of the ``k = 8`` elementwise budget and 7 more than a stored operand: ``(n + 12) * 2u * mag`` with ``mag`` the
  weight-gradient of ``|x|`` and ``|A|*sum|dp| + |B*y| + |C|``.

* The 16-bit fused stem weight gradients (``wgrad_stem_rows`` / ``wgrad_stem_quad``) form dY = A*dz + B*y + C per 2x2
  quad in fp32 (dz: up to 4 pooled gradients added in window order, then two fmas: at most 5 roundings per term, inside
  the ``12u * dymag`` of stem_pool_bwd_apply) and ROUND IT TO 16 BITS (``E::pack2``) into the LDS tile the MFMA reads:
  the operand is off by ``e_i = half_ulp16(dY_i) + 12u * dymag_i`` from the fp64 dY.  That error is carried through the
  sum, the accumulation adds the usual term:
  ``|dw - ref| <= sum_i |x_i| * e_i + (n + 4) * 2u * sum_i |x_i| * (|dY_i| + e_i)`` (``stem_fused_bound``).  The ReLU mask
  is not recomputed there: it is in the argmax bytes (a dead window carries 255), so the operands' argmax must agree with
  y (``cc.stem_fused_operands``).  Integer operands: dY is a multiple of 1/2 below 32, exact in both 16-bit types, so
  the result equals the fp64 reference.

* fp16 SUBNORMAL operands (|v| < 2**-14; they occur in unscaled fp16 gradients) lower the accuracy of the MFMA's own
  sum: the unit aligns the products of one instruction by the operands' exponent FIELDS, and a subnormal's field says
  2**-14 whatever its leading zeros, so a term is kept to one fp32 ulp of the largest NOMINAL product
  ``max(|x|, 2**-14) * max(|dy|, 2**-14)``, not of the largest true one (measured on the MI355X through ``conv_wgrad`` with
  12-term sums: x ~ N(0, 1) against dY ~ 2**-16 * N(0, 1) errs by up to 1.9 * 2u * mag where normal operands give
  0.9 and bf16 0.5; single products are exact at every exponent pair, nothing is flushed).  The model for a sum with
  fp16 operands that may be subnormal is therefore the same ``(n + 4) * 2u * mag`` with ``mag`` taken over the nominal
  magnitudes (``conv_wgrad_nominal_mag``; a zero -- padding included -- counts as 2**-14 too: its field is the same).
  Normal operands have nominal = true magnitude: the bound is unchanged for them, and bf16 has no subnormals in range.
  Only the fp32-output weight gradient can see the difference; a 16-bit output's own rounding (at least 2**-25) hides it.

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
import torch.nn.functional as F

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


def assert_within(got, ref64, bound64, name="value", C=None, family=None, shape=None) -> float:
    """|got - ref| <= bound for every element; the message names the worst element, its channel, error and bound (and,
    with ``shape``, its index in a tensor of that shape, e.g. (n, h, w, channel))."""
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
        if shape is not None:
            ch += f", index {tuple(int(v) for v in torch.unravel_index(torch.tensor(i), tuple(shape)))}"
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


def xent_ref(logits, bias, tgt, ncls, gs, dtype):
    """fp64 reference of the fused cross entropy over the first ``ncls`` columns of the 16-bit (or fp32) ``logits``
    [B, ld] (bounds: tests/test_small_kernels_gpu.py docstring): dict v (logit + bias) and vmag, loss and loss_bound per
    row, dlogits = (softmax - onehot) * gs and dlogits_bound, correct (first maximum of the fp32 logit + bias == target)."""
    l64 = logits[:, :ncls].double()
    b64 = bias.double() if bias is not None else torch.zeros(ncls, dtype=torch.float64, device=logits.device)
    v64 = l64 + b64
    loss = F.cross_entropy(v64, tgt, reduction="none")
    d = (torch.softmax(v64, 1) - F.one_hot(tgt, ncls)) * gs
    v32 = logits[:, :ncls].float() + (bias if bias is not None else 0.0)  # the fp32 values the kernel compares
    ar = torch.arange(ncls, device=logits.device).expand_as(v32)
    first = torch.where(v32 == v32.max(1, keepdim=True).values, ar, torch.full_like(ar, ncls)).min(1).values
    return dict(v=v64, vmag=l64.abs() + b64.abs(), loss=loss,
                loss_bound=2.0 ** -18 * (1 + v64.abs().max(1).values + loss.abs()), dlogits=d,
                dlogits_bound=half_ulp16(d, dtype) + 2.0 ** -18 * gs, correct=(first == tgt).float())


def finalize_carried(ref, ds, dss, count, gamma, eps, momentum):
    """How far forward-finalize outputs may move when the sums they are made from are off by ``ds`` (sum x) and ``dss``
    (sum x^2) per channel -- the step audit feeds ``bn_finalize_ref`` the fp64 sums of the stored y, the kernel its own
    fp32-chained statistics of the same y (``assert_conv_stats``'s allowance).  First principles, no linearisation:
    mean moves by em = ds/count; the biased variance sum x^2/count - mean^2 by ev = dss/count + 2|mean|em + em^2 (the
    clamp at 0 is 1-Lipschitz); invstd = f(var) = (var + eps)^-1/2 is decreasing and convex, so it moves by at most
    ei = f(max(var - ev, 0)) - f(var); scale by |gamma| ei; shift = beta - mean * scale by em|scale| + |mean| es + em es;
    the running statistics' new terms by momentum * em and momentum * ev * count/(count - 1)."""
    eps32 = float(torch.tensor(eps, dtype=torch.float32).item())
    mom = float(torch.tensor(momentum, dtype=torch.float32).item())
    em = ds / count
    ev = dss / count + 2 * ref["mean"].abs() * em + em * em
    ei = 1.0 / torch.sqrt((ref["var"] - ev).clamp_min(0.0) + eps32) - ref["invstd"]
    es = gamma.to(torch.float64).abs() * ei
    return dict(mean=em, var=ev, invstd=ei, scale=es, shift=em * ref["scale"].abs() + ref["mean"].abs() * es + em * es,
                rm=mom * em, rv=mom * ev * (count / (count - 1) if count > 1 else 1.0))


def check_finalize_carried(coef, rm, rv, ref, car, C, name, family=None):
    """``check_finalize`` with the statistics' own error ``car`` (``finalize_carried``) carried into every output: each
    bound is the carried movement e plus the rounding term of ``check_finalize`` taken at |ref| + e."""
    w = 0.0
    ab = lambda k: ref[k].abs()
    w = max(w, assert_within(coef[2 * C:3 * C], ref["mean"], car["mean"] + 2 * U * (ab("mean") + car["mean"]),
                             f"{name}: mean", C, family))
    w = max(w, assert_within(coef[3 * C:4 * C], ref["invstd"], car["invstd"] + 4 * U * (ab("invstd") + car["invstd"]),
                             f"{name}: invstd", C, family))
    w = max(w, assert_within(coef[:C], ref["scale"], car["scale"] + 4 * U * (ab("scale") + car["scale"]),
                             f"{name}: scale", C, family))
    w = max(w, assert_within(coef[C:2 * C], ref["shift"], car["shift"] + 6 * U * (
        ab("beta") + (ref["mean"] * ref["scale"]).abs() + car["shift"]), f"{name}: shift", C, family))
    if rm is not None:
        w = max(w, assert_within(rm, ref["rm_old"] + ref["rm_new"], car["rm"] + 6 * U * (
            ab("rm_old") + ab("rm_new") + car["rm"]), f"{name}: running_mean", C, family))
        w = max(w, assert_within(rv, ref["rv_old"] + ref["rv_new"], car["rv"] + 6 * U * (
            ab("rv_old") + ab("rv_new") + car["rv"]), f"{name}: running_var", C, family))
    return w


def check_bwd_finalize_carried(bcoef, dgamma, dbeta, ref, b0, b1, count, gscale, coef, C, name, family=None):
    """``check_bwd_finalize`` where the kernel's sums may differ from the reference sums by ``b0`` (sum dz) and ``b1``
    (sum dz*xhat) per channel (``assert_bnb_sums``'s bounds): dbeta / dgamma move by gscale * b0 / b1; A does not
    depend on the sums; B = -A*invstd*sdzx/count by |A*invstd| b1/count; Cc = -A*sdz/count + A*invstd*mean*sdzx/count
    by |A| b0/count + |A*invstd*mean| b1/count.  The rounding terms of ``check_bwd_finalize`` are taken at |ref| + e."""
    c64 = coef.to(torch.float64)
    mean, invstd = c64[2 * C:3 * C], c64[3 * C:4 * C]
    A = ref["A"].abs()
    eB = A * invstd.abs() * b1 / count
    eC = A * b0 / count + A * (invstd * mean).abs() * b1 / count
    w = 0.0
    if dgamma is not None:
        e = gscale * b1
        w = max(w, assert_within(dgamma, ref["dgamma"], e + 2 * U * (ref["dgamma"].abs() + e), f"{name}: dgamma", C, family))
    if dbeta is not None:
        e = gscale * b0
        w = max(w, assert_within(dbeta, ref["dbeta"], e + 2 * U * (ref["dbeta"].abs() + e), f"{name}: dbeta", C, family))
    w = max(w, assert_within(bcoef[:C], ref["A"], 4 * U * A, f"{name}: bcoef A", C, family))
    w = max(w, assert_within(bcoef[C:2 * C], ref["B"], eB + 6 * U * (ref["B"].abs() + eB), f"{name}: bcoef B", C, family))
    w = max(w, assert_within(bcoef[2 * C:3 * C], ref["Cc"], eC + 8 * U * (ref["Cmag"] + eC), f"{name}: bcoef C", C, family))
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


# ------------------------------------------------------------------------------------- convolutions (NHWC / KRSC)
def _out_hw(H, W, R, S, stride, pad):
    return (H + 2 * pad - R) // stride + 1, (W + 2 * pad - S) // stride + 1


def _unfold_matmul(x64, wmat64, R, S, stride, pad):
    """x64 [N, C, H, W], wmat64 [K, C*R*S] -> [N, K, L] (float64 im2col + matmul, the same code on CPU and GPU)."""
    return torch.matmul(wmat64, F.unfold(x64, (R, S), padding=pad, stride=stride))


def conv_fwd_ref(x, w, stride, pad, residual=None):
    """fp64 y = conv(x, w) (+ residual) of NHWC ``x`` [N, H, W, C] and KRSC ``w`` [K, R, S, C] -> (ref, mag), both
    [N, P, Q, K]; ``mag`` is the same operation on the absolute values of the operands."""
    N, H, W, C = x.shape
    K, R, S, _ = w.shape
    P, Q = _out_hw(H, W, R, S, stride, pad)
    x64 = x.to(torch.float64).permute(0, 3, 1, 2)
    wm = w.to(torch.float64).permute(0, 3, 1, 2).reshape(K, C * R * S)
    ref = _unfold_matmul(x64, wm, R, S, stride, pad).view(N, K, P, Q).permute(0, 2, 3, 1).contiguous()
    mag = _unfold_matmul(x64.abs(), wm.abs(), R, S, stride, pad).view(N, K, P, Q).permute(0, 2, 3, 1).contiguous()
    if residual is not None:
        r64 = residual.to(torch.float64).view_as(ref)
        ref, mag = ref + r64, mag + r64.abs()
    return ref, mag


def dgrad_as_correlation(dy, w, H, W, stride, pad, ftype):
    """The data gradient as a stride-1 correlation: (zero-dilated, zero-padded dY [N, K, H+R-1, W+S-1], weight matrix
    [C, K*R*S] with wt[c][k][r][s] = w[k][R-1-r][S-1-s][c]) in float type ``ftype``."""
    N, P, Q, K = dy.shape
    K2, R, S, C = w.shape
    assert K == K2
    top, left = R - 1 - pad, S - 1 - pad
    Hd, Wd = H + R - 1, W + S - 1  # a stride-1 R x S window over this extent gives H x W outputs
    assert top >= 0 and left >= 0
    # dY rows beyond the extent would only meet inputs the forward conv never read
    assert top + (P - 1) * stride < Hd and left + (Q - 1) * stride < Wd, "dY exceeds the forward geometry"
    dil = torch.zeros(N, K, Hd, Wd, dtype=ftype, device=dy.device)
    dil[:, :, top:top + (P - 1) * stride + 1:stride, left:left + (Q - 1) * stride + 1:stride] = \
        dy.to(ftype).permute(0, 3, 1, 2)
    return dil, w.to(ftype).flip(1, 2).permute(3, 0, 1, 2).reshape(C, K * R * S)


def conv_dgrad_ref(dy, w, H, W, stride, pad, residual=None, res_phase=None):
    """fp64 dX [N, H, W, C] of y = conv(x, w) given dY [N, P, Q, K] and KRSC ``w`` -> (ref, mag): the stride-1
    correlation of the zero-dilated, zero-padded dY with the flipped, transposed weight.  ``residual`` has dX's shape,
    or, with ``res_phase = (ph, pw)``, is compact [N, ceil((H-ph)/stride), ceil((W-pw)/stride), C] and is added on the
    pixels (ph + stride*i, pw + stride*j) only."""
    N, P, Q, K = dy.shape
    R, S, C = w.shape[1:]
    dil, wm = dgrad_as_correlation(dy, w, H, W, stride, pad, torch.float64)
    ref = _unfold_matmul(dil, wm, R, S, 1, 0).view(N, C, H, W).permute(0, 2, 3, 1).contiguous()
    mag = _unfold_matmul(dil.abs(), wm.abs(), R, S, 1, 0).view(N, C, H, W).permute(0, 2, 3, 1).contiguous()
    if residual is not None:
        r64 = residual.to(torch.float64)
        if res_phase is not None:
            ph, pw = res_phase
            full = torch.zeros_like(ref)
            full[:, ph::stride, pw::stride] = r64.view(N, -(-(H - ph) // stride), -(-(W - pw) // stride), C)
            r64 = full
        r64 = r64.view_as(ref)
        ref, mag = ref + r64, mag + r64.abs()
    return ref, mag


def conv_wgrad_ref(x, dy, R, S, stride, pad):
    """fp64 dW [K, R, S, C] of y = conv(x, w) from NHWC ``x`` and dY [N, P, Q, K] -> (ref, mag)."""
    N, H, W, C = x.shape
    _, P, Q, K = dy.shape
    assert (P, Q) == _out_hw(H, W, R, S, stride, pad)
    x64 = x.to(torch.float64).permute(0, 3, 1, 2)
    d64 = dy.to(torch.float64).reshape(N, P * Q, K)

    def one(xa, da):
        cols = F.unfold(xa, (R, S), padding=pad, stride=stride)  # [N, C*R*S, L]
        dw = torch.matmul(cols, da).sum(0)  # [C*R*S, K]
        return dw.view(C, R, S, K).permute(3, 1, 2, 0).contiguous()
    return one(x64, d64), one(x64.abs(), d64.abs())


FP16_MIN_NORMAL = 2.0 ** -14


def nominal16(v, dtype):
    """|v| as the MFMA's alignment sees a 16-bit operand (module docstring): fp16 values below the smallest normal
    number, zero included, count as 2**-14."""
    a = v.to(torch.float64).abs()
    return a.clamp_min(FP16_MIN_NORMAL) if dtype == torch.float16 else a


def conv_wgrad_nominal_mag(x, dy, R, S, stride, pad, dtype):
    """``conv_wgrad_ref``'s mag [K, R, S, C] over the nominal operand magnitudes (``nominal16``; the zero padding of an
    fp16 image counts as 2**-14): equal to the plain mag where every operand is a normal number."""
    N, H, W, C = x.shape
    _, P, Q, K = dy.shape
    fill = FP16_MIN_NORMAL if dtype == torch.float16 else 0.0
    xn = F.pad(nominal16(x, dtype).permute(0, 3, 1, 2), (pad, pad, pad, pad), value=fill)
    cols = F.unfold(xn, (R, S), padding=0, stride=stride)
    dw = torch.matmul(cols, nominal16(dy, dtype).reshape(N, P * Q, K)).sum(0)
    return dw.view(C, R, S, K).permute(3, 1, 2, 0).contiguous()


def conv_int_operands(shape, values, seed):
    """A float32 CPU tensor of ``shape`` drawn uniformly from the integers ``values`` (CPU generator: the CPU test and
    the GPU test see the same numbers)."""
    g = torch.Generator().manual_seed(seed)
    v = torch.tensor(values, dtype=torch.float32)
    return v[torch.randint(len(values), tuple(shape), generator=g)]


INT_RANGE = {torch.bfloat16: 256.0, torch.float16: 2048.0,  # |integer| up to here is exactly representable
             torch.float32: 2.0 ** 24}


def int_case_conditions(ref64, dtype, K):
    """The layer-A conditions on a reference alone: (share of outputs outside the exactly representable integer range of
    ``dtype``, largest per-channel sum of squares of the rounded outputs)."""
    share = float((ref64.abs() > INT_RANGE[dtype]).double().mean().item())
    y = ref64.to(torch.float32).to(dtype).to(torch.float64).reshape(-1, K)
    return share, float((y * y).sum(0).max().item())


def conv_bound(ref64, mag64, n, dtype):
    """Element bound of a 16-bit conv output (dtype float32: of an fp32 one): half_ulp16(ref) + (n + 4)*2u*mag."""
    return half_ulp16(ref64, dtype) + (n + 4) * 2 * U * mag64.abs()


def assert_conv(out, ref64, mag64, n, dtype, name, family):
    """Every element of a forward / data-gradient (16-bit) or weight-gradient (``dtype`` float32) result within
    ``conv_bound``; the failure names the element's index (n, h, w, channel)."""
    return assert_within(out, ref64, conv_bound(ref64, mag64, n, dtype), name, ref64.shape[-1], family, ref64.shape)


def stem_fused_bound(x, dy64, dymag64, n, dtype):
    """Element bound [64, 7, 7, 3] of the 16-bit fused stem weight gradient (module docstring): ``x`` the NHWC image the
    kernel reads, ``dy64`` / ``dymag64`` the fp64 dY [N, P, Q, 64] and the sum of the absolute values of its terms."""
    e = half_ulp16(dy64, dtype) + 12 * U * dymag64
    _, carried = conv_wgrad_ref(x, e, 7, 7, 2, 3)
    _, mag = conv_wgrad_ref(x, dy64.abs() + e, 7, 7, 2, 3)
    return carried + (n + 4) * 2 * U * mag


def conv32_bound(mag64, n, extra=5):
    """Element bound of an fp32 MFMA conv output: (n + 5)*2u*mag (``extra`` = 12: the fused stem weight gradient)."""
    return (n + extra) * 2 * U * mag64.abs()


def assert_conv32(out, ref64, mag64, n, name, family, extra=5):
    """Every element of an fp32 forward / data-gradient / weight-gradient result within ``conv32_bound``."""
    return assert_within(out, ref64, conv32_bound(mag64, n, extra), name, ref64.shape[-1], family, ref64.shape)


def int32_case_conditions(ref64, mag64, K):
    """The fp32 integer layer's conditions on a reference alone: (largest magnitude bound of a partial sum, largest
    per-channel sum of squares of the outputs); both must stay below 2**24."""
    y = ref64.reshape(-1, K)
    return float(mag64.max().item()), float((y * y).sum(0).max().item())


def wide_operand(shape, bits, seed):
    """fp32 CPU tensor of random-sign odd integers with exactly ``bits`` significant bits (2**(bits-1)+1 ..
    2**bits - 1): every bit of the significand field in use matters, the lowest included."""
    g = torch.Generator().manual_seed(seed)
    half = torch.randint(2 ** (bits - 2), 2 ** (bits - 1), tuple(shape), generator=g)  # 2*half + 1 is odd, top bit set
    sign = torch.randint(0, 2, tuple(shape), generator=g) * 2 - 1
    return ((2 * half + 1) * sign).to(torch.float32)


def wide_small(shape, seed):
    """fp32 CPU tensor from +-{1, 2, 4}: a product with it is exact and keeps every bit of the other operand."""
    return conv_int_operands(shape, (-4, -2, -1, 1, 2, 4), seed)


def round_to_bits(t, bits):
    """``t`` (fp32) rounded to ``bits`` significand bits, to nearest even (the mutation of the ``wide`` proofs)."""
    m, e = torch.frexp(t.double())
    return torch.ldexp(torch.round(m * 2.0 ** bits) / 2.0 ** bits, e).float()


def assert_exact(out, expect, name):
    """Layer A: ``out`` equals ``expect`` (fp64 integers already rounded to the output type) in every element; the
    failure names the element, its index and the got / expected values."""
    assert out.shape == expect.shape, f"{name}: shapes {tuple(out.shape)} {tuple(expect.shape)}"
    return assert_within(out, expect, 0.0, name, expect.shape[-1], None, expect.shape)


def round_exact(ref64, dtype):
    """The one rounding layer A allows: fp64 integers -> fp32 (exact) -> the output type, back in fp64."""
    return ref64.to(torch.float32).to(dtype).to(torch.float64)


def assert_conv_stats(s, ss, y, name, family="conv16_stats", exact=False):
    """Forward statistics against fp64 sums of the kernel's stored ``y`` [..., K]: the reduction alone (chain bound with
    n_chain = rows; ``exact``: equal)."""
    K = y.shape[-1]
    y64 = y.to(torch.float64).reshape(-1, K)
    rows = y64.shape[0]
    r0, r1 = y64.sum(0), (y64 * y64).sum(0)
    if exact:
        return max(assert_within(s, r0, 0.0, f"{name}: sum", K), assert_within(ss, r1, 0.0, f"{name}: sumsq", K))
    return max(assert_sum(s, r0, y64.abs().sum(0), rows, f"{name}: sum", K, family),
               assert_sum(ss, r1, r1, rows, f"{name}: sumsq", K, family))


def bn_xhat(y, coef, C):
    """fp64 xhat = (y - mean) * invstd from the fp32 coefficients [scale | shift | mean | invstd] the kernel reads."""
    c64 = coef.to(torch.float64)
    return (y.to(torch.float64).reshape(-1, C) - c64[2 * C:3 * C]) * c64[3 * C:4 * C]


def assert_bnb_sums(got_dz, got_dzx, dz_ref64, bound64, xhat64, name, family="conv16_bnb_sums", exact=False):
    """Fused BN-backward sums against the independent reference: ``dz_ref64`` [rows, C] (masked fp64 data gradient;
    ``exact``: already rounded to the output type), ``bound64`` the element bound of dz (zero where masked)."""
    rows, C = dz_ref64.shape
    t = dz_ref64 * xhat64
    r0, r1 = dz_ref64.sum(0), t.sum(0)
    if exact:
        return max(assert_within(got_dz, r0, 0.0, f"{name}: sum dz", C),
                   assert_within(got_dzx, r1, 0.0, f"{name}: sum dz*xhat", C))
    b0 = bound64.sum(0) + (rows + 4) * U * dz_ref64.abs().sum(0)
    b1 = (bound64 * xhat64.abs()).sum(0) + (rows + 4) * U * t.abs().sum(0)
    return max(assert_within(got_dz, r0, b0, f"{name}: sum dz", C, family),
               assert_within(got_dzx, r1, b1, f"{name}: sum dz*xhat", C, family))
