"""The 3x3/2 first-conv (csrc/kernels/stem3x3.hip) cases shared by tests/test_stem3x3_cpu.py (the cases and the
assertions proven on references and on mutations of a torch emulation) and tests/test_stem3x3_gpu.py (the kernels):
one list, so they cannot drift apart (a plain module).

A geometry is ``(N, H, W, K)``: fp32 NHWC image [N, H, W, 3], KRSC weight [K, 3, 3, 3], output [N, P, Q, K] with
``P = (H - 1) // 2 + 1``; as a conv geometry of tests/_conv_cases.py it is ``(N, H, W, 3, K, 3, 2, 1)``, which is where
operands come from; references and magnitudes are tests/_numerics.py's.  Three layers:

* ``int``   (layer A) integers: the result must come out bit for bit;
* ``real``  (layer B) reals already rounded to the 16-bit dtype, inside ``assert_conv``'s bound with ``n`` the reduction
  length (27 forward, M = N*P*Q for the fp32 weight gradient);
* ``round`` the in-kernel rounding: a plain fp32 ``randn`` image that is NOT representable in 16 bits, judged by the
  same bound against the reference of ``x.to(dtype)`` (round to nearest even), the value the kernel must form.

* ``tiny``  weight gradient, fp16 only (``TINY_GEOMS``): dY is the ``real`` operand times 2**-16, which is subnormal in
  fp16 (|dy| < 4) and nonzero unless |dy| < 2**-9 -- the unscaled fp16 gradients the torch engine hands the kernel.  The
  MFMA keeps such a sum to an ulp of the NOMINAL magnitudes (tests/_numerics.py): judged by ``assert_conv`` over
  ``conv_wgrad_nominal_mag``.

The kernel is always handed an fp32 image: ``d["x32"]``.
"""
import torch
import torch.nn.functional as F

import _conv_cases as cc
import _numerics as nm

DTYPES = cc.DTYPES
LAYERS = ["int", "real", "round"]

GEOMS = [
    (1, 1, 2, 8),        # one output pixel
    (1, 3, 3, 8),        # small odd sides
    (2, 8, 8, 16),       # even sides: no bottom / right padding read
    (2, 9, 7, 24),       # odd sides: bottom row and right column of padding
    (3, 10, 13, 32),     # mixed parity, M = 105
    (1, 32, 32, 40),     # K = 8 mod 16
    (2, 20, 18, 64),     # widest K
    (5, 17, 15, 48),     # tiles crossing rows and images, M = 360
    (1, 6, 300, 16),     # an output row longer than a pixel tile
    (4, 56, 56, 32),     # weight gradient with one split and with many
]
WGRAD_PLAN_GEOM = (4, 56, 56, 32)
ISOLATION_GEOMS = [(2, 9, 7, 24), (5, 17, 15, 48)]
WGRAD_TARGETS = [None, 1, 4096]  # None: the op's default
RED, RED_PAD = 27, 32            # the reduction and its MFMA K-step
TINY_GEOMS = [(2, 9, 7, 24), (3, 10, 13, 32)]
TINY_SCALE = 2.0 ** -16


def conv_geom(g):
    N, H, W, K = g
    return (N, H, W, 3, K, 3, 2, 1)


def out_hw(g):
    return (g[1] - 1) // 2 + 1, (g[2] - 1) // 2 + 1


def rows(g):
    P, Q = out_hw(g)
    return g[0] * P * Q


_cache = {}


def _round_image(g, salt):
    N, H, W, K = g
    gen = torch.Generator().manual_seed(cc._seed(conv_geom(g), salt))
    return torch.randn(N, H, W, 3, generator=gen)


def case(kind, g, dtype, layer):
    """Operands (CPU) and the fp64 reference of one pass of one geometry, made once and shared (read-only) by every
    test: dict with ``x32`` (the fp32 image the kernel reads), ``x`` (the 16-bit image the reference is made of:
    ``x32.to(dtype)``), ``w`` [K, 3, 3, 3] (fwd) or ``dy`` [N, P, Q, K] (wgrad), ``ref``, ``mag`` and ``n``."""
    key = (kind, g, dtype, layer)
    if key in _cache:
        return _cache[key]
    cg = conv_geom(g)
    src = "real" if layer in ("round", "tiny") else layer
    if kind == "fwd":
        x, w, _ = cc.fwd_operands(cg, dtype, src)
        x32 = _round_image(g, 101) if layer == "round" else x.float()
        x = x32.to(dtype)
        ref, mag = nm.conv_fwd_ref(x, w, 2, 1)
        d = dict(x32=x32, x=x, w=w, ref=ref, mag=mag, n=RED)
    else:
        x, dy = cc.wgrad_operands(cg, dtype, src)
        x32 = _round_image(g, 102) if layer == "round" else x.float()
        x = x32.to(dtype)
        if layer == "tiny":
            assert dtype == torch.float16, "the tiny layer is fp16 only"
            dy = (dy.float() * TINY_SCALE).to(dtype)
        ref, mag = nm.conv_wgrad_ref(x, dy, 3, 3, 2, 1)
        if layer == "tiny":
            mag = nm.conv_wgrad_nominal_mag(x, dy, 3, 3, 2, 1, dtype)
        d = dict(x32=x32, x=x, dy=dy, ref=ref, mag=mag, n=rows(g))
    _cache[key] = d
    return d


def judge(out, d, dtype, layer, name, family):
    """The layers' verdict on a 16-bit forward output; returns the worst error / bound ratio."""
    assert out.shape == d["ref"].shape, (name, tuple(out.shape), tuple(d["ref"].shape))
    if layer == "int":
        return nm.assert_exact(out, nm.round_exact(d["ref"], dtype), name)
    return nm.assert_conv(out, d["ref"], d["mag"], d["n"], dtype, name, family)


def judge_dw(dw, d, layer, name, family="stem3x3_wgrad"):
    """The same for the fp32 weight gradient [K, 3, 3, 3] (KRSC): layer A equals the reference."""
    assert dw.dtype == torch.float32 and dw.shape == d["ref"].shape, (name, dw.dtype, tuple(dw.shape))
    if layer == "int":
        return nm.assert_exact(dw, d["ref"], name)
    return nm.assert_conv(dw, d["ref"], d["mag"], d["n"], torch.float32, name, family)


# ---- the torch emulation of a correct kernel: the image rounded to the dtype, an fp32 unfold (the patch matrix in the
# kernel's own order, j = (r * 3 + s) * 3 + c, padded with zeros to 32 slots) and an fp32 matmul rounded once; the
# weight gradient stays fp32 and is summed split by split, in split order, as wgrad_reduce does.  The keyword arguments
# are the mutations tests/test_stem3x3_cpu.py proves the cases on.
def truncate16(x32, dtype):
    """fp32 -> 16 bits toward zero (the mutation of round-to-nearest-even)."""
    if dtype == torch.bfloat16:
        return (x32.contiguous().view(torch.int32) & -65536).view(torch.float32).to(dtype)
    r = x32.to(dtype)
    over = r.float().abs() > x32.abs()
    return torch.where(over, (r.view(torch.int16) - 1).view(dtype), r)


def patches(x32, dtype, drop_tap=None, pad0=False, real_bottom=False, real_right=False, reverse_c=False,
            truncate=False, slot27=0.0):
    """[M, 32] fp32 patch matrix of the image as the kernel must form it."""
    N, H, W, _ = x32.shape
    P, Q = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    x = (truncate16(x32, dtype) if truncate else x32.to(dtype)).float()
    if reverse_c:
        x = x.flip(-1)
    xn = x.permute(0, 3, 1, 2)
    top = 0 if pad0 else 1  # pad0: the window starts at (2p, 2q) instead of (2p - 1, 2q - 1)
    xp = F.pad(xn, (top, 3, top, 3))
    if real_bottom and not pad0:  # the row below the image repeats its last row instead of being padding
        xp[:, :, H + 1] = xp[:, :, H]
    if real_right and not pad0:
        xp[:, :, :, W + 1] = xp[:, :, :, W]
    out = torch.zeros(N, P, Q, RED_PAD)
    for r in range(3):
        for s in range(3):
            if drop_tap == (r, s):
                continue
            tap = xp[:, :, r:r + 2 * P - 1:2, s:s + 2 * Q - 1:2]  # [N, 3, P, Q]
            out[..., (r * 3 + s) * 3:(r * 3 + s) * 3 + 3] = tap.permute(0, 2, 3, 1)
    out[..., RED] = slot27
    return out.reshape(N * P * Q, RED_PAD)


def emul_fwd(x32, w, dtype, neighbour_w=False, **mut):
    N, H, W, _ = x32.shape
    K = w.shape[0]
    wm = torch.zeros(K, RED_PAD)
    wm[:, :RED] = w.float().reshape(K, RED)
    if neighbour_w:  # channel k computed with channel k + 1's weights
        wm = wm.roll(-1, 0)
    y = patches(x32, dtype, **mut) @ wm.t()
    return y.to(dtype).reshape(N, (H - 1) // 2 + 1, (W - 1) // 2 + 1, K)


def emul_wgrad(x32, dy, dtype, pix_per_split, drop_last_split=False, swap_rs=False, **mut):
    K = dy.shape[-1]
    pm, df = patches(x32, dtype, **mut), dy.float().reshape(-1, K)
    M = pm.shape[0]
    starts = list(range(0, M, pix_per_split))
    if drop_last_split:
        starts = starts[:-1]
    dw = torch.zeros(K, RED_PAD)
    for s in starts:
        dw = dw + df[s:s + pix_per_split].t() @ pm[s:s + pix_per_split]
    dw = dw[:, :RED].reshape(K, 3, 3, 3)
    return (dw.transpose(1, 2) if swap_rs else dw).contiguous()
