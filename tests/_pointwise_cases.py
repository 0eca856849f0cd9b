"""The pointwise-conv (csrc/kernels/pwconv.hip) cases shared by tests/test_pointwise_cpu.py (the cases and the
assertions proven on references and on mutations of a torch emulation) and tests/test_pointwise_gpu.py (the kernels):
one list, so they cannot drift apart (a plain module).

A geometry is ``(N, H, W, C, K)``: NHWC input [N, H, W, C], weight [K, C]; as a conv geometry of tests/_conv_cases.py
it is ``(N, H, W, C, K, 1, 1, 0)``, which is where operands come from; references and magnitudes are
tests/_numerics.py's.  Both layers of that module apply: layer A (integers) must come out bit for bit, layer B (reals)
within ``assert_conv``'s bound with ``n`` the reduction length (C forward, K backward data, M = N*H*W weight gradient).

A third layer, ``tiny``, exists for the weight gradient in fp16 only (``TINY_GEOMS``): dY is the ``real`` operand times
2**-16, which is subnormal in fp16 (|dy| < 4) and nonzero unless |dy| < 2**-9 -- the unscaled fp16 gradients the torch
engine hands the kernel.  The MFMA keeps such a sum to an ulp of the NOMINAL magnitudes (tests/_numerics.py): the layer
is judged by ``assert_conv`` over ``conv_wgrad_nominal_mag``.
"""
import torch

import _conv_cases as cc
import _numerics as nm

DTYPES = cc.DTYPES
LAYERS = ["int", "real"]

GEOMS = [
    (2, 5, 7, 8, 8),         # minimum widths
    (3, 9, 11, 16, 96),      # MobileNetV2's first expansion, ragged M = 297
    (2, 7, 9, 96, 24),       # 24-channel output tail
    (2, 6, 6, 24, 144),      # reduction of 24 (one partial K-step), K = 128 + 16
    (1, 3, 5, 144, 32),      # reduction 4 * 32 + 16
    (5, 13, 13, 40, 200),    # both = 8 mod 16, M = 845 (several tiles plus a tail)
    (2, 4, 4, 960, 320),     # long reduction
    (2, 2, 2, 320, 1280),    # widest, several output slices
    (1, 1, 1, 32, 16),       # M = 1
    (1, 2, 3, 2048, 8),      # contract limit
    (1, 2, 3, 8, 2048),      # contract limit
    (4, 28, 28, 32, 192),    # weight gradient with one split and with many
]
WGRAD_PLAN_GEOM = (4, 28, 28, 32, 192)
ISOLATION_GEOMS = [(2, 6, 6, 24, 144), (5, 13, 13, 40, 200)]
WGRAD_TARGETS = [None, 1, 4096]  # None: the op's default
TINY_GEOMS = [(3, 9, 11, 16, 96), (1, 3, 5, 144, 32)]  # the two smallest with a ragged reduction
TINY_SCALE = 2.0 ** -16


def conv_geom(g):
    N, H, W, C, K = g
    return (N, H, W, C, K, 1, 1, 0)


def rows(g):
    return g[0] * g[1] * g[2]


_cache = {}


def case(kind, g, dtype, layer):
    """Operands (CPU, in ``dtype``) and the fp64 reference of one pass of one geometry, made once and shared
    (read-only) by every test: dict with the operands, ``ref``, ``mag`` and ``n`` (the reduction length).
    kind "fwd": x [N, H, W, C], w [K, C], ref [N, H, W, K]; "dgrad": dy [N, H, W, K], w [K, C], ref [N, H, W, C];
    "wgrad": x, dy, ref [K, C] (layer "tiny": module docstring; ``mag`` is then the nominal one)."""
    key = (kind, g, dtype, layer)
    if key in _cache:
        return _cache[key]
    N, H, W, C, K = g
    cg = conv_geom(g)
    if kind == "fwd":
        x, w, _ = cc.fwd_operands(cg, dtype, layer)
        ref, mag = nm.conv_fwd_ref(x, w, 1, 0)
        d = dict(x=x, w=w.reshape(K, C), ref=ref, mag=mag, n=C)
    elif kind == "dgrad":
        dy, w, _ = cc.dgrad_operands(cg, dtype, layer)
        ref, mag = nm.conv_dgrad_ref(dy, w, H, W, 1, 0)
        d = dict(dy=dy, w=w.reshape(K, C), ref=ref, mag=mag, n=K)
    else:
        x, dy = cc.wgrad_operands(cg, dtype, "real" if layer == "tiny" else layer)
        if layer == "tiny":
            assert dtype == torch.float16, "the tiny layer is fp16 only"
            dy = (dy.float() * TINY_SCALE).to(dtype)
        ref, mag = nm.conv_wgrad_ref(x, dy, 1, 1, 1, 0)
        if layer == "tiny":
            mag = nm.conv_wgrad_nominal_mag(x, dy, 1, 1, 1, 0, dtype)
        d = dict(x=x, dy=dy, ref=ref.reshape(K, C), mag=mag.reshape(K, C), n=rows(g))
    _cache[key] = d
    return d


def judge(out, d, dtype, layer, name, family):
    """The two layers' verdict on a 16-bit forward / backward-data output; returns the worst error / bound ratio."""
    assert out.shape == d["ref"].shape, (name, tuple(out.shape), tuple(d["ref"].shape))
    if layer == "int":
        return nm.assert_exact(out, nm.round_exact(d["ref"], dtype), name)
    return nm.assert_conv(out, d["ref"], d["mag"], d["n"], dtype, name, family)


def judge_dw(dw, d, layer, name, family="pwconv_wgrad"):
    """The same for the fp32 weight gradient [K, C]: layer A equals the reference."""
    assert dw.dtype == torch.float32 and dw.shape == d["ref"].shape, (name, dw.dtype, tuple(dw.shape))
    if layer == "int":
        return nm.assert_exact(dw, d["ref"], name)
    return nm.assert_conv(dw, d["ref"], d["mag"], d["n"], torch.float32, name, family)


# ---- the torch emulation of a correct kernel: a plain fp32 matmul rounded once (the weight gradient stays fp32 and is
# summed split by split, in split order, as wgrad_reduce does)
def emul_fwd(x, w, dtype):
    return (x.float().reshape(-1, w.shape[1]) @ w.float().t()).to(dtype).reshape(x.shape[:-1] + (w.shape[0],))


def emul_dgrad(dy, w, dtype):
    return (dy.float().reshape(-1, w.shape[0]) @ w.float()).to(dtype).reshape(dy.shape[:-1] + (w.shape[1],))


def emul_wgrad(x, dy, pix_per_split, drop_last_split=False):
    C, K = x.shape[-1], dy.shape[-1]
    xf, df = x.float().reshape(-1, C), dy.float().reshape(-1, K)
    M = xf.shape[0]
    starts = list(range(0, M, pix_per_split))
    if drop_last_split:
        starts = starts[:-1]
    dw = torch.zeros(K, C)
    for s in starts:
        dw = dw + df[s:s + pix_per_split].t() @ xf[s:s + pix_per_split]
    return dw
