"""Every 16-bit MFMA conv route per element against an independent fp64 reference (run on an MI355X).

Two layers per route and dtype (tests/_numerics.py derives the bounds, tests/_conv_cases.py holds the cases and the
operands, tests/test_numerics_model_cpu.py proves that the assertions bite):

* layer ``int``: operands from {-2, -1, 1, 2} x {-1, 1}.  Every partial sum is an integer far below 2**24, so the fp32
  accumulator is exact in any order, grouping, split or tile walk and the result must equal the fp64 reference rounded
  once to the output type, bit for bit: any mismatch is a dropped, doubled or misplaced term.
* layer ``real``: randn operands, every element within ``half_ulp16(ref) + (n + 4) * 2u * mag``: this layer owns
  rounding-mode and scaling errors.

No reference comes from a kernel of this project: outputs are compared with ``F.unfold`` + ``matmul`` in float64 on the
16-bit values the kernel reads, statistics with fp64 sums of the stored output, and the fused BN-backward sums with
sums over the independent ``dz``.  Outputs are pre-filled with NaN and every test asserts through the dispatch
counters that the route it names ran.
"""
import pytest
import torch

import _conv_cases as cc
import _numerics as nm

pytestmark = pytest.mark.gpu

DEV = "cuda"
LAYERS = ["int", "real"]
TILES = [(128, 128, 64), (256, 64, 64), (128, 64, 64), (64, 128, 64), (256, 128, 64), (256, 256, 32),
         (128, 128, 32), (256, 64, 32), (128, 64, 32), (256, 256, 64), (512, 128, 64), (256, 128, 32)]
PP_TILES = [(256, 256, 64), (512, 128, 64)]
SPECIAL = ("conv_l1_fwd", "conv_l1_dgrad", "conv_l1_pp", "conv_l1_sliced", "conv1x1_c64", "conv1x1_c64_bnb", "conv1x1x",
           "conv1x1x_bnb")

_cache = {}


def _cached(key, make):
    if key not in _cache:
        if len(_cache) > 6:  # the references of a few cases at a time: tests of one case run next to each other
            _cache.pop(next(iter(_cache)))
        _cache[key] = make()
    return _cache[key]


def _dev(t):
    return None if t is None else t.to(DEV).contiguous()


def _C():
    from pytorch_distributed_template_amd.ops import native
    return native.C


def _nan(*shape, dtype):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def _slots(C, K, q=2):
    return torch.zeros(C.stat_slots() * K * q, dtype=torch.float64, device=DEV)


class _Counts:
    """with _Counts() as c: ...; c.n(key): how often the route ran inside the block."""

    def __enter__(self):
        _C().reset_dispatch_counts()
        return self

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        self.d = dict(_C().dispatch_counts())
        return False

    def n(self, key):
        return self.d.get(key, 0)

    def none_of(self, keys):
        hit = {k: self.d[k] for k in keys if self.d.get(k, 0)}
        assert not hit, f"a specialised route ran: {hit}"


# ------------------------------------------------------------------------------------------------ cases (cached)
def _fwd_case(g, dtype, layer, residual=False):
    def make():
        x, w, res = cc.fwd_operands(g, dtype, layer, narrow=g in cc.NARROW, residual=residual)
        x, w, res = _dev(x), _dev(w), _dev(res)
        ref, mag = nm.conv_fwd_ref(x, w, g[6], g[7], res)
        return dict(x=x, w=w, res=res, ref=ref, mag=mag, n=g[3] * g[5] * g[5])
    return _cached(("fwd", g, dtype, layer, residual), make)


def _dgrad_case(g, dtype, layer, residual=None):
    def make():
        dy, w, res = cc.dgrad_operands(g, dtype, layer, residual, narrow=g in cc.NARROW)
        dy, w, res = _dev(dy), _dev(w), _dev(res)
        ref, mag = nm.conv_dgrad_ref(dy, w, g[1], g[2], g[6], g[7], res, (0, 0) if residual == "compact" else None)
        return dict(dy=dy, w=w, res=res, ref=ref, mag=mag, n=g[4] * g[5] * g[5])
    return _cached(("dgrad", g, dtype, layer, residual), make)


def _wgrad_case(g, dtype, layer):
    def make():
        x, dy = cc.wgrad_operands(g, dtype, layer)
        x, dy = _dev(x), _dev(dy)
        ref, mag = nm.conv_wgrad_ref(x, dy, g[5], g[5], g[6], g[7])
        P, Q = cc.out_hw(g)
        return dict(x=x, dy=dy, ref=ref, mag=mag, n=g[0] * P * Q)
    return _cached(("wgrad", g, dtype, layer), make)


# --------------------------------------------------------------------------------------------------- launches
def _run_fwd(x, w, stride, pad, stats=False, residual=None, tile=None, max_wg=0):
    """ops.conv.conv_fwd over a NaN-filled output: (y, sums [K, 2] or None)."""
    from pytorch_distributed_template_amd.ops import conv
    C = _C()
    N, H, W, Ci = x.shape
    K, R, S, _ = w.shape
    P, Q = conv.out_hw(H, W, R, S, stride, pad)
    y = _nan(N, P, Q, K, dtype=x.dtype)
    bm, bn = conv.conv_tile(K, Ci * R * S, N * P * Q)
    bk = 64 if Ci % 64 == 0 else 32
    if tile is not None:
        bm, bn, bk = tile
    sp = _slots(C, K) if stats else None
    C.conv_fwd(x, w, y, residual, sp, N, H, W, Ci, K, R, S, P, Q, stride, stride, -pad, -pad, 1, 1, P, Q, 1, 1, 0, 0,
               bm, bn, bk, 0, max_wg)
    return y, (sp.view(-1, K, 2).sum(0) if stats else None), (bm, bn, bk)


def _run_dgrad(dy, w, H, W, stride, pad, residual=None, bnb=None, tile=None, res_phase=-1, max_wg=0):
    """ops.conv.conv_dgrad over a NaN-filled output: (dx, (bm, bn, bk), number of phases)."""
    from pytorch_distributed_template_amd.ops import conv
    C = _C()
    N, P, Q, K = dy.shape
    _, R, S, Ci = w.shape
    dx = _nan(N, H, W, Ci, dtype=dy.dtype)
    bm, bn = conv.conv_tile(Ci, K * R * S, N * H * W)
    bk = 64 if K % 64 == 0 else 32
    if tile is not None:
        bm, bn, bk = tile
    wflat = w.reshape(-1)
    pieces, phases, off = [], [], 0
    for ph, pw, rs, ss, ioff_h, ioff_w in conv.dgrad_phases(R, S, stride, pad):
        if H - ph <= 0 or W - pw <= 0:
            continue
        idx = conv.dgrad_weight_index(K, Ci, R, S, rs, ss).to(w.device)
        if idx.numel():
            pieces.append(wflat[idx])
        phases.append([ph, pw, len(rs), len(ss), ioff_h, ioff_w, off])
        off += idx.numel()
    wt = torch.cat(pieces).contiguous()
    C.conv_dgrad_bn(dy, wt, dx, residual, N, P, Q, K, Ci, H, W, stride, phases, bm, bn, bk,
                    *(bnb or (0, None, None, None, None, None, None)), res_phase, max_wg)
    return dx, (bm, bn, bk), len(phases)


def _run_wgrad(x, dy, R, stride, pad, target, pre=None):
    C = _C()
    N, H, W, Ci = x.shape
    _, P, Q, K = dy.shape
    splits, pps, tile = C.conv_wgrad_plan(K, R, R, Ci, N * P * Q, target, False)
    ldw = R * R * Ci
    ws = _nan(splits * K * ldw, dtype=torch.float32)
    C.conv_wgrad(x, dy, ws, N, H, W, Ci, K, R, R, P, Q, stride, stride, pad, pad, 1, 1, ldw, splits, pps, 0, False,
                 pre=pre)
    out = _nan(K * ldw, dtype=torch.float32)
    C.wgrad_reduce(ws, splits, K, ldw, ldw, K * ldw, out, ldw, 1.0, False)
    return out.view(K, R, R, Ci), tile


def _is_pp(tile, cin):
    bm, bn, bk = tile
    return bk == 64 and cin % 64 == 0 and (bm, bn) in ((256, 256), (512, 128))


def _assert_generic_or_pp(c, tile, cin, dgrad, nphase=1):
    """The tiled implicit-GEMM kernel this tile names ran once, and no specialised kernel."""
    c.none_of(SPECIAL)
    if _is_pp(tile, cin):
        key = "conv_pp_dgrad" if dgrad else "conv_pp_fwd"
    elif dgrad:
        key = "conv_generic_dgrad_phased" if nphase > 1 else "conv_generic_dgrad"
    else:
        key = "conv_generic_fwd"
    assert c.n(key) == 1, (key, c.d)


# ----------------------------------------------------------------------------------------------------- checks
def _rec(family, dtype, worst):
    """The family's ratio per dtype as well (RATIOS[family] is kept by the assertion itself)."""
    key = f"{family}/{str(dtype).split('.')[-1]}"
    nm.RATIOS[key] = max(nm.RATIOS.get(key, 0.0), worst)


def _check16(out, case, layer, dtype, name, family):
    ref, mag = case["ref"], case["mag"]
    assert out.shape == ref.shape, f"{name}: shape {tuple(out.shape)} vs {tuple(ref.shape)}"
    if layer == "int":
        share, _ = nm.int_case_conditions(ref, dtype, ref.shape[-1])
        assert share <= 0.01, f"{name}: {share:.4f} of the reference lies outside the exact integer range"
        nm.assert_exact(out, nm.round_exact(ref, dtype), name)
    else:
        _rec(family, dtype, nm.assert_conv(out, ref, mag, case["n"], dtype, name, family))


def _check_stats(sums, y, case, layer, dtype, name):
    if layer == "int":
        assert nm.int_case_conditions(case["ref"], dtype, y.shape[-1])[1] < 2.0 ** 24
    worst = nm.assert_conv_stats(sums[:, 0], sums[:, 1], y, name, exact=layer == "int")
    if layer != "int":
        _rec("conv16_stats", dtype, worst)


def _check_wgrad(dw, case, layer, name, dtype):
    if layer == "int":
        nm.assert_exact(dw, case["ref"].float().double(), name)
        assert torch.equal(dw, case["ref"].float())
    else:
        _rec("conv16_wgrad", dtype,
             nm.assert_conv(dw, case["ref"], case["mag"], case["n"], torch.float32, name, "conv16_wgrad"))


def _bnb_args(mode, shape, dtype, layer):
    """(the conv_dgrad bnb tuple, the operands on the device, the slots)."""
    from pytorch_distributed_template_amd.ops import conv
    d = {k: _dev(v) for k, v in cc.bnb_operands(mode, shape, dtype, layer).items()}
    Cc = shape[-1]
    slots = _slots(_C(), Cc, 4 if mode == 3 else 2)
    om = conv.pack_relu_mask(d["out"]) if mode > 1 else None
    return (mode, d["y1"], d["coef1"], d["y2"], d["coef2"], om, slots), d, slots


def _check_bnb(mode, dz, slots, case, d, layer, dtype, name):
    """dz = dgrad_ref * mask per element, and sum dz, sum dz * xhat (both branches) against sums over that reference."""
    Cc = case["ref"].shape[-1]
    KO = 4 if mode == 3 else 2
    sums = slots.view(-1, Cc, KO).sum(0)
    mask, unsure = cc.bnb_mask(mode, d, Cc)
    ref = torch.where(mask, case["ref"].reshape(-1, Cc), torch.zeros((), dtype=torch.float64, device=DEV))
    x1 = nm.bn_xhat(d["y1"], d["coef1"], Cc)
    x2 = nm.bn_xhat(d["y2"], d["coef2"], Cc) if mode == 3 else None
    if layer == "int":
        assert not bool(unsure.any())
        share, _ = nm.int_case_conditions(case["ref"], dtype, Cc)
        assert share <= 0.01
        exp = nm.round_exact(ref, dtype)
        nm.assert_exact(dz.reshape(-1, Cc), exp, f"{name}: dz")
        nm.assert_bnb_sums(sums[:, 0], sums[:, 1], exp, None, x1, f"{name}: branch 1", exact=True)
        if mode == 3:
            nm.assert_bnb_sums(sums[:, 2], sums[:, 3], exp, None, x2, f"{name}: branch 2", exact=True)
        return
    full = nm.conv_bound(case["ref"], case["mag"], case["n"], dtype).reshape(-1, Cc)
    bound = torch.where(mask, full, torch.zeros_like(full))
    share = float(unsure.double().mean().item())
    assert share <= 1e-3, f"{name}: {share:.5f} of the pre-activations are too close to zero to call"
    # elements whose ReLU sign fp32 may call either way: left out of the element comparison, and either value
    # (0 or the data gradient) is accepted inside the sums
    got = torch.where(unsure, ref, dz.reshape(-1, Cc).double())
    _rec("conv16_dgrad", dtype, nm.assert_within(got, ref, bound, f"{name}: dz", Cc, "conv16_dgrad", ref.shape))
    sb = torch.where(unsure, case["ref"].reshape(-1, Cc).abs() + full, bound)
    _rec("conv16_bnb_sums", dtype, nm.assert_bnb_sums(sums[:, 0], sums[:, 1], ref, sb, x1, f"{name}: branch 1"))
    if mode == 3:
        _rec("conv16_bnb_sums", dtype, nm.assert_bnb_sums(sums[:, 2], sums[:, 3], ref, sb, x2, f"{name}: branch 2"))


def _res_kind(mode):
    return None if mode == 1 else "full"


# ============================================================================ generic ring kernel, every tile
@pytest.mark.parametrize("layer", LAYERS)
@pytest.mark.parametrize("dtype", cc.DTYPES)
@pytest.mark.parametrize("tile", TILES)
def test_every_tile_forward_stats_and_dgrad_residual(tile, dtype, layer):
    """Strided 3x3, 15 x 13, 256 -> 256 on every compiled tile: ragged M tail, four dgrad phases of unequal size."""
    g = cc.TILE_GEOM
    N, H, W, Ci, K, R, st, pad = g
    f = _fwd_case(g, dtype, layer)
    with _Counts() as c:
        y, sums, _ = _run_fwd(f["x"], f["w"], st, pad, stats=True, tile=tile)
    _assert_generic_or_pp(c, tile, Ci, False)
    _check16(y, f, layer, dtype, f"fwd tile {tile}", "conv16_fwd")
    _check_stats(sums, y, f, layer, dtype, f"fwd tile {tile}")
    d = _dgrad_case(g, dtype, layer, "full")
    with _Counts() as c:
        dx, _, nph = _run_dgrad(d["dy"], d["w"], H, W, st, pad, residual=d["res"], tile=tile)
    _assert_generic_or_pp(c, tile, K, True, nph)
    _check16(dx, d, layer, dtype, f"dgrad tile {tile}", "conv16_dgrad")


# ============================================================================ default dispatch (conv_tile)
@pytest.mark.parametrize("layer", LAYERS)
@pytest.mark.parametrize("dtype", cc.DTYPES)
@pytest.mark.parametrize("g", cc.DEFAULT_GEOMS)
def test_default_dispatch_forward_stats_and_dgrad_residual(g, dtype, layer):
    N, H, W, Ci, K, R, st, pad = g
    f = _fwd_case(g, dtype, layer)
    with _Counts() as c:
        y, sums, tile = _run_fwd(f["x"], f["w"], st, pad, stats=True)
    _assert_generic_or_pp(c, tile, Ci, False)
    _check16(y, f, layer, dtype, f"fwd {g}", "conv16_fwd")
    _check_stats(sums, y, f, layer, dtype, f"fwd {g}")
    d = _dgrad_case(g, dtype, layer, "full")
    with _Counts() as c:
        dx, tile, nph = _run_dgrad(d["dy"], d["w"], H, W, st, pad, residual=d["res"])
    _assert_generic_or_pp(c, tile, K, True, nph)
    _check16(dx, d, layer, dtype, f"dgrad {g}", "conv16_dgrad")
    if R == 1 and st == 2:  # the phases without taps hold the residual alone
        assert nph == 4


# ============================================================================ persistent ping-pong kernel
@pytest.mark.parametrize("layer", LAYERS)
@pytest.mark.parametrize("dtype", cc.DTYPES)
@pytest.mark.parametrize("max_wg", [1, 4096])
@pytest.mark.parametrize("tile", PP_TILES)
@pytest.mark.parametrize("g", cc.PP_GEOMS)
def test_pingpong_forward_stats(g, tile, max_wg, dtype, layer):
    """One workgroup walking every tile (prefetched K-step 0 at each boundary) and one tile per workgroup."""
    N, H, W, Ci, K, R, st, pad = g
    f = _fwd_case(g, dtype, layer)
    with _Counts() as c:
        y, sums, _ = _run_fwd(f["x"], f["w"], st, pad, stats=True, tile=tile, max_wg=max_wg)
    assert c.n("conv_pp_fwd") == 1 and c.n("conv_pp_512x128") == (tile[0] == 512), c.d
    c.none_of(SPECIAL + ("conv_generic_fwd",))
    _check16(y, f, layer, dtype, f"pp fwd {g} {tile} max_wg={max_wg}", "conv16_fwd")
    _check_stats(sums, y, f, layer, dtype, f"pp fwd {g} {tile}")


@pytest.mark.parametrize("layer", LAYERS)
@pytest.mark.parametrize("dtype", cc.DTYPES)
@pytest.mark.parametrize("max_wg", [1, 4096])
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("tile", PP_TILES)
def test_pingpong_dgrad_every_epilogue(tile, mode, max_wg, dtype, layer):
    """Stride-1 3x3 256 -> 256 backward data: plain with residual (mode 0) and the three fused BN-backward epilogues."""
    g = cc.PP_GEOMS[0]
    N, H, W, Ci, K, R, st, pad = g
    d = _dgrad_case(g, dtype, layer, "full" if mode == 0 else _res_kind(mode))
    name = f"pp dgrad mode {mode} {tile} max_wg={max_wg}"
    if mode == 0:
        with _Counts() as c:
            dx, _, _ = _run_dgrad(d["dy"], d["w"], H, W, st, pad, residual=d["res"], tile=tile, max_wg=max_wg)
        assert c.n("conv_pp_dgrad") == 1 and c.n("conv_dgrad_bn_reduce_epilogue") == 0, c.d
        _check16(dx, d, layer, dtype, name, "conv16_dgrad")
        return
    bnb, ops, slots = _bnb_args(mode, (N, H, W, Ci), dtype, layer)
    with _Counts() as c:
        dz, _, _ = _run_dgrad(d["dy"], d["w"], H, W, st, pad, residual=d["res"], bnb=bnb, tile=tile, max_wg=max_wg)
    assert c.n("conv_pp_dgrad") == 1 and c.n("conv_dgrad_bn_reduce_epilogue") == 1, c.d
    c.none_of(SPECIAL)
    _check_bnb(mode, dz, slots, d, ops, layer, dtype, name)


@pytest.mark.parametrize("layer", LAYERS)
@pytest.mark.parametrize("dtype", cc.DTYPES)
@pytest.mark.parametrize("max_wg", [1, 4096])
@pytest.mark.parametrize("mode", [0, 2])
def test_pingpong_dgrad_strided_compact_residual(mode, max_wg, dtype, layer):
    """3x3/2, 15 x 13, 256 -> 512 backward data with a compact residual on phase 0 (and the block-output epilogue):
    phase 0 has two tiles, the other phases one."""
    g = cc.PP_STRIDED_GEOM
    N, H, W, Ci, K, R, st, pad = g
    tile = (256, 256, 64)
    d = _dgrad_case(g, dtype, layer, "compact")
    name = f"pp strided dgrad mode {mode} max_wg={max_wg}"
    bnb, ops, slots = _bnb_args(mode, (N, H, W, Ci), dtype, layer) if mode else (None, None, None)
    with _Counts() as c:
        dz, _, nph = _run_dgrad(d["dy"], d["w"], H, W, st, pad, residual=d["res"], bnb=bnb, tile=tile, res_phase=0,
                                max_wg=max_wg)
    assert nph == 4 and c.n("conv_pp_dgrad") == 1 and c.n("conv_dgrad_compact_residual") == 1, c.d
    if mode == 0:
        _check16(dz, d, layer, dtype, name, "conv16_dgrad")
    else:
        assert c.n("conv_dgrad_bn_reduce_epilogue") == 1
        _check_bnb(mode, dz, slots, d, ops, layer, dtype, name)


# ============================================================================ layer1 halo kernel (conv_l1)
def _pre_case(g, dtype, layer):
    """conv over relu(bn(z)) with the producer BN + ReLU fused into the kernel: the reference convolves the 16-bit
    rounding of the fp32 fma, zero padded AFTER the transform."""
    def make():
        z, w, _ = cc.fwd_operands(g, dtype, layer)
        coef = cc.pre_operands(layer, dtype)
        z, w, coef = _dev(z), _dev(w), _dev(coef)
        a = cc.pre_apply_ref(z, coef, dtype).float().to(dtype)
        ref, mag = nm.conv_fwd_ref(a, w, g[6], g[7])
        return dict(z=z, w=w, coef=coef, a=a, ref=ref, mag=mag, n=g[3] * g[5] * g[5])
    return _cached(("pre", g, dtype, layer), make)


@pytest.mark.parametrize("layer", LAYERS)
@pytest.mark.parametrize("dtype", cc.DTYPES)
@pytest.mark.parametrize("variant", ["fwd", "fwd_stats", "fwd_pre", "dgrad_res", "dgrad_bn1", "dgrad_bn2"])
@pytest.mark.parametrize("pp", [0, 1])
@pytest.mark.parametrize("g", cc.L1_GEOMS)
def test_conv_l1_4wave_and_8wave(g, pp, variant, dtype, layer):
    C = _C()
    N, H, W, Ci, K, R, st, pad = g
    name = f"conv_l1 pp={pp} {variant} {g}"
    old = C.conv_l1_set_pp(pp)
    try:
        if variant.startswith("fwd"):
            if variant == "fwd_pre":
                f = _pre_case(g, dtype, layer)
                y, sp = _nan(N, H, W, K, dtype=dtype), _slots(C, K)
                with _Counts() as c:
                    C.conv_fwd_pre(f["z"], f["w"], y, sp, f["coef"], N, H, W)
                assert c.n("conv_l1_fwd_fused_bn_relu") == 1, c.d
                sums = sp.view(-1, K, 2).sum(0)
            else:
                f = _fwd_case(g, dtype, layer)
                with _Counts() as c:
                    y, sums, _ = _run_fwd(f["x"], f["w"], st, pad, stats=variant == "fwd_stats")
            assert c.n("conv_l1_fwd") == 1 and c.n("conv_l1_pp") == pp and c.n("conv_generic_fwd") == 0, c.d
            _check16(y, f, layer, dtype, name, "conv16_fwd")
            if sums is not None:
                _check_stats(sums, y, f, layer, dtype, name)
            return
        mode = {"dgrad_res": 0, "dgrad_bn1": 1, "dgrad_bn2": 2}[variant]
        d = _dgrad_case(g, dtype, layer, "full" if mode == 0 else _res_kind(mode))
        bnb, ops, slots = _bnb_args(mode, (N, H, W, Ci), dtype, layer) if mode else (None, None, None)
        with _Counts() as c:
            dz, _, _ = _run_dgrad(d["dy"], d["w"], H, W, st, pad, residual=d["res"], bnb=bnb)
        assert c.n("conv_l1_dgrad") == 1 and c.n("conv_l1_pp") == pp and c.n("conv_generic_dgrad") == 0, c.d
        if mode == 0:
            _check16(dz, d, layer, dtype, name, "conv16_dgrad")
        else:
            _check_bnb(mode, dz, slots, d, ops, layer, dtype, name)
    finally:
        C.conv_l1_set_pp(old)


@pytest.mark.parametrize("layer", LAYERS)
@pytest.mark.parametrize("dtype", cc.DTYPES)
def test_conv_l1_partial_row_tiles_fall_to_the_generic_kernel(dtype, layer):
    g = cc.L1_FALLBACK_GEOM
    N, H, W, Ci, K, R, st, pad = g
    f = _fwd_case(g, dtype, layer)
    with _Counts() as c:
        y, sums, tile = _run_fwd(f["x"], f["w"], st, pad, stats=True)
    _assert_generic_or_pp(c, tile, Ci, False)
    _check16(y, f, layer, dtype, f"fwd {g}", "conv16_fwd")
    _check_stats(sums, y, f, layer, dtype, f"fwd {g}")
    d = _dgrad_case(g, dtype, layer, "full")
    with _Counts() as c:
        dx, tile, nph = _run_dgrad(d["dy"], d["w"], H, W, st, pad, residual=d["res"])
    _assert_generic_or_pp(c, tile, K, True, nph)
    _check16(dx, d, layer, dtype, f"dgrad {g}", "conv16_dgrad")


# ============================================================================ persistent 1x1 64 -> 256 (conv1x1.hip)
@pytest.mark.parametrize("layer", LAYERS)
@pytest.mark.parametrize("dtype", cc.DTYPES)
@pytest.mark.parametrize("variant", ["plain", "stats", "fused_bn_relu"])
@pytest.mark.parametrize("M", cc.C64_M)
def test_conv1x1_c64_forward(M, variant, dtype, layer):
    C = _C()
    if not C.conv1x1_c64_supported(64, 256):
        pytest.skip("PDT_CONV1X1=0")
    if variant == "fused_bn_relu" and layer == "int" and M == 70005:
        # relu(bn(z)) >= 0 gives the outputs a mean: over 70005 rows a channel's sum of squares passes 2**24, so the
        # exact layer runs the fused form at the 12581 rows of test_fused_producer_bn_relu_1x1_c64 (99 tiles, a 37-row
        # tail); the real layer keeps 70005
        M = cc.C64_FUSED_INT_M
    g = cc.c64_geom(M)
    f = _pre_case(g, dtype, layer) if variant == "fused_bn_relu" else _fwd_case(g, dtype, layer)
    y = _nan(1, 1, M, 256, dtype=dtype)
    sp = _slots(C, 256) if variant != "plain" else None
    with _Counts() as c:
        if variant == "fused_bn_relu":
            C.conv1x1_c64(f["z"], f["w"], y, sp, M, pre=f["coef"])
        else:
            C.conv1x1_c64(f["x"], f["w"], y, sp, M)
    assert c.n("conv1x1_c64") == 1 and c.n("conv1x1_c64_fused_bn_relu") == (variant == "fused_bn_relu"), c.d
    assert c.n("conv_generic_fwd") == 0
    name = f"conv1x1_c64 {variant} M={M}"
    _check16(y, f, layer, dtype, name, "conv16_fwd")
    if sp is not None:
        _check_stats(sp.view(-1, 256, 2).sum(0), y, f, layer, dtype, name)


@pytest.mark.parametrize("layer", LAYERS)
@pytest.mark.parametrize("dtype", cc.DTYPES)
@pytest.mark.parametrize("sliced", [0, 1])
@pytest.mark.parametrize("nhw,mode,cin", cc.C64_BNB)
def test_conv1x1_c64_dgrad_block_output_epilogue(nhw, mode, cin, sliced, dtype, layer):
    """ResNet-50 layer1's 1x1 256 -> 64 | 128 backward data on the dedicated kernel (conv1x1.hip) and on the sliced
    kernel's C = 64 configurations (conv1x1x_l1_mode 1)."""
    C = _C()
    if not C.conv1x1_c64_supported(64, 256):
        pytest.skip("PDT_CONV1X1=0")
    g = cc.bnb_1x1_geom(nhw, cin, 256)
    N, H, W = nhw
    d = _dgrad_case(g, dtype, layer, "full")
    bnb, ops, slots = _bnb_args(mode, (N, H, W, 256), dtype, layer)
    prev = C.conv1x1x_l1_mode(sliced)
    try:
        with _Counts() as c:
            dz, _, _ = _run_dgrad(d["dy"], d["w"], H, W, 1, 0, residual=d["res"], bnb=bnb)
    finally:
        C.conv1x1x_l1_mode(prev)
    assert c.n("conv1x1_c64_bnb") == 1 - sliced and c.n("conv1x1x_bnb") == sliced, c.d
    assert c.n("conv_generic_dgrad") == 0
    _check_bnb(mode, dz, slots, d, ops, layer, dtype, f"conv1x1_c64_bnb {nhw} mode {mode} cin {cin} sliced {sliced}")


# ============================================================================ persistent sliced 1x1 (conv1x1x.hip)
@pytest.mark.parametrize("layer", LAYERS)
@pytest.mark.parametrize("dtype", cc.DTYPES)
@pytest.mark.parametrize("cin,M", cc.X_PLAIN)
def test_conv1x1x_forward_stats(cin, M, dtype, layer):
    C = _C()
    if not C.conv1x1x_supported(cin, 4 * cin):
        pytest.skip("PDT_CONV1X1X=0")
    f = _fwd_case(cc.x_plain_geom(cin, M), dtype, layer)
    for stats in (False, True):
        y = _nan(1, 1, M, 4 * cin, dtype=dtype)
        sp = _slots(C, 4 * cin) if stats else None
        with _Counts() as c:
            C.conv1x1x(f["x"], f["w"], y, sp, M, cin, 4 * cin, 1, 0, 0, 0)
        assert c.n("conv1x1x") == 1 and c.n("conv1x1x_strided") == 0 and c.n("conv_generic_fwd") == 0, c.d
        _check16(y, f, layer, dtype, f"conv1x1x cin={cin} M={M}", "conv16_fwd")
        if stats:
            _check_stats(sp.view(-1, 4 * cin, 2).sum(0), y, f, layer, dtype, f"conv1x1x cin={cin} M={M}")


@pytest.mark.parametrize("layer", LAYERS)
@pytest.mark.parametrize("dtype", cc.DTYPES)
@pytest.mark.parametrize("cin,nhw", cc.X_STRIDED)
def test_conv1x1x_strided_forward_stats(cin, nhw, dtype, layer):
    C = _C()
    if not C.conv1x1x_supported(cin, 2 * cin):
        pytest.skip("PDT_CONV1X1X=0")
    g = cc.x_strided_geom(cin, nhw)
    f = _fwd_case(g, dtype, layer)
    N, H, W = nhw
    P, Q = cc.out_hw(g)
    M = N * P * Q
    y = _nan(N, P, Q, 2 * cin, dtype=dtype)
    sp = _slots(C, 2 * cin)
    with _Counts() as c:
        C.conv1x1x(f["x"], f["w"], y, sp, M, cin, 2 * cin, 2, N, H, W)
    assert c.n("conv1x1x_strided") == 1 and c.n("conv_generic_fwd") == 0, c.d
    _check16(y, f, layer, dtype, f"conv1x1x strided cin={cin} {nhw}", "conv16_fwd")
    _check_stats(sp.view(-1, 2 * cin, 2).sum(0), y, f, layer, dtype, f"conv1x1x strided cin={cin} {nhw}")


@pytest.mark.parametrize("layer", LAYERS)
@pytest.mark.parametrize("dtype", cc.DTYPES)
@pytest.mark.parametrize("mode", [2, 3])
@pytest.mark.parametrize("cin,nhw", cc.X_BNB)
def test_conv1x1x_dgrad_block_output_epilogue(cin, nhw, mode, dtype, layer):
    C = _C()
    Co = 4 * cin
    g = cc.bnb_1x1_geom(nhw, cin, Co)
    N, H, W = nhw
    d = _dgrad_case(g, dtype, layer, "full")
    bnb, ops, slots = _bnb_args(mode, (N, H, W, Co), dtype, layer)
    prev = C.conv1x1x_mode(1)
    try:
        with _Counts() as c:
            dz, _, _ = _run_dgrad(d["dy"], d["w"], H, W, 1, 0, residual=d["res"], bnb=bnb)
    finally:
        C.conv1x1x_mode(prev)
    assert c.n("conv1x1x_bnb") == 1 and c.n("conv1x1x_bnb_2br") == (mode == 3) and c.n("conv_generic_dgrad") == 0, c.d
    _check_bnb(mode, dz, slots, d, ops, layer, dtype, f"conv1x1x_bnb cin={cin} {nhw} mode {mode}")


# ============================================================================ grouped conv, every slice in one launch
@pytest.mark.parametrize("layer", LAYERS)
@pytest.mark.parametrize("dtype", cc.DTYPES)
@pytest.mark.parametrize("width,groups,stride,H", cc.GROUPED)
def test_grouped_slices_one_launch(width, groups, stride, H, dtype, layer):
    """blockIdx.z = slice: forward with statistics, backward data (plain and with the inner-BN reduce) and the weight
    gradient against the dense block-diagonal reference -- a term leaking from another slice is a wrong integer."""
    from pytorch_distributed_template_amd.ops import conv
    C = _C()
    g = cc.grouped_geom(width, groups, stride, H)
    N, _, W, _, _, R, _, pad = g
    P, Q = cc.out_hw(g)
    S, nsl = 64, width // 64

    def make():
        _, dense, full = cc.grouped_weights(width, groups, dtype, layer)
        x, _, _ = cc.fwd_operands(g, dtype, layer)
        dy, _, _ = cc.dgrad_operands(g, dtype, layer)
        x, dy, dense, full = _dev(x), _dev(dy), _dev(dense), _dev(full)
        fr, fm = nm.conv_fwd_ref(x, full, stride, pad)
        dr, dm = nm.conv_dgrad_ref(dy, full, H, W, stride, pad)
        wr, wm = nm.conv_wgrad_ref(x, dy, R, R, stride, pad)
        return dict(x=x, dy=dy, dense=dense, fwd=dict(ref=fr, mag=fm, n=S * 9), dg=dict(ref=dr, mag=dm, n=S * 9),
                    wg=dict(ref=wr, mag=wm, n=N * P * Q))
    k = _cached(("grouped", g, groups, dtype, layer), make)
    x, dy, dense = k["x"], k["dy"], k["dense"]
    name = f"grouped {width}/{groups} stride {stride} H {H}"
    y, st = _nan(N, P, Q, width, dtype=dtype), _slots(C, width)
    with _Counts() as c:
        C.gconv_fwd(x, dense.reshape(-1), y, st, N, H, W, width, R, stride, pad, P, Q, -1, 256, 64)
    c.none_of(SPECIAL)
    assert c.n("gconv_fwd") == 1, c.d
    _check16(y, k["fwd"], layer, dtype, f"{name}: fwd", "conv16_fwd")
    _check_stats(st.view(-1, width, 2).sum(0), y, k["fwd"], layer, dtype, f"{name}: fwd")
    # backward data: the phase weights of every dense slice weight, slice after slice
    derived, phases, off = [], [], 0
    for j in range(nsl):
        flat = dense[j].reshape(-1)
        for ph, pw, rs, ss, ioff_h, ioff_w in conv.dgrad_phases(R, R, stride, pad):
            m = conv.dgrad_weight_index(S, S, R, R, rs, ss)
            if m.numel() == 0 or H - ph <= 0 or W - pw <= 0:
                continue
            derived.append(flat[m.to(DEV)])
            if j == 0:
                phases.append([ph, pw, len(rs), len(ss), ioff_h, ioff_w, off])
            off += m.numel()
    derived = torch.cat(derived)
    dx = _nan(N, H, W, width, dtype=dtype)
    with _Counts() as c:
        C.gconv_dgrad(dy, derived, dx, N, P, Q, width, H, W, stride, phases, -1, 256, 64)
    c.none_of(SPECIAL)
    assert c.n("gconv_dgrad") == 1, c.d
    _check16(dx, k["dg"], layer, dtype, f"{name}: dgrad", "conv16_dgrad")
    bnb, ops, slots = _bnb_args(1, (N, H, W, width), dtype, layer)
    dz = _nan(N, H, W, width, dtype=dtype)
    with _Counts() as c:
        C.gconv_dgrad(dy, derived, dz, N, P, Q, width, H, W, stride, phases, -1, 256, 64, bn_y1=ops["y1"],
                      bn_coef1=ops["coef1"], bn_slots=slots)
    assert c.n("gconv_dgrad") == 1 and c.n("conv_dgrad_bn_reduce_epilogue") == 1, c.d
    _check_bnb(1, dz, slots, k["dg"], ops, layer, dtype, f"{name}: dgrad + BN reduce")
    # weight gradient: the diagonal 64 x 64 blocks of the dense dW
    splits, pps, _ = C.conv_wgrad_plan(S, R, R, S, N * P * Q, 256, False)
    ldw = R * R * S
    ws = _nan(splits * nsl * S * ldw, dtype=torch.float32)
    with _Counts() as c:
        C.gconv_wgrad(x, dy, ws, N, H, W, width, R, P, Q, stride, pad, -1, ldw, splits, pps)
    assert c.n("gconv_wgrad") == 1 and c.n("conv_wgrad_generic") == 1, c.d
    dwd = _nan(nsl * S * ldw, dtype=torch.float32)
    C.wgrad_reduce(ws, splits, nsl * S, ldw, ldw, nsl * S * ldw, dwd, ldw, 1.0, False)
    dwd = dwd.view(nsl, S, R, R, S)
    blocks = lambda t: torch.stack([t[j * S:(j + 1) * S, :, :, j * S:(j + 1) * S] for j in range(nsl)])
    diag = dict(ref=blocks(k["wg"]["ref"]), mag=blocks(k["wg"]["mag"]), n=k["wg"]["n"])
    _check_wgrad(dwd, diag, layer, f"{name}: wgrad", dtype)


# ============================================================================ stem (stem_pack + stem_fwd)
@pytest.mark.parametrize("layer", LAYERS)
@pytest.mark.parametrize("dtype", cc.DTYPES)
@pytest.mark.parametrize("N,blocks_per_cu", [(cc.STEM[0][0], 2), (0, 1)])
def test_stem_window_mode(N, blocks_per_cu, dtype, layer):
    """7x7/2 pad-3 stem over the zero-padded NHWC4 image; N = 0: the smallest batch with more 4-row tiles than blocks
    (the persistent loop with its next-tile prefetch)."""
    C = _C()
    H = W = 32
    K = 64
    P = Q = 16
    if N == 0:
        N = cc.STEM[1][0]
        assert N * (P // 4) > torch.cuda.get_device_properties(0).multi_processor_count * blocks_per_cu
    Hp, Wp = max(H + 6, 2 * (P - 1) + 8), max(W + 6, 2 * (Q - 1) + 8)

    def make():
        x, wk = cc.stem_operands(N, H, W, dtype, layer)
        x, wk = _dev(x), _dev(wk.to(dtype))
        xr = x.to(dtype).permute(0, 2, 3, 1).contiguous()  # what stem_pack stores (round to nearest even)
        ref, mag = nm.conv_fwd_ref(xr, wk, 2, 3)
        return dict(x=x, wk=wk, ref=ref, mag=mag, n=7 * 32)
    k = _cached(("stem", N, dtype, layer), make)
    xp = _nan(N * Hp * Wp * 4, dtype=dtype)
    C.stem_pack(k["x"], xp, N, 3, H, W, 3, Hp, Wp)
    wwin = torch.zeros(K, 7, 8, 4, dtype=dtype, device=DEV)
    wwin[:, :, :7, :3] = k["wk"]
    wwin = wwin.reshape(K, 7 * 32).contiguous()
    y, st = _nan(N, P, Q, K, dtype=dtype), _slots(C, K)
    with _Counts() as c:
        C.stem_fwd(xp, wwin, y.view(-1), st, N, Hp, Wp, P, Q, blocks_per_cu)
    assert c.n("stem_fwd") == 1, c.d
    _check16(y, k, layer, dtype, f"stem_fwd N={N}", "conv16_fwd")
    _check_stats(st.view(-1, K, 2).sum(0), y, k, layer, dtype, f"stem_fwd N={N}")
    if N == 3:  # the same conv on the generic kernel's window mode (one kernel row per tap)
        y2 = _nan(N, P, Q, K, dtype=dtype)
        with _Counts() as c:
            C.conv_fwd(xp, wwin, y2.view(-1), None, None, N, Hp, Wp, 32, K, 7, 1, P, Q, 2, 2, 0, 0, 1, 0, P, Q, 1, 1,
                       0, 0, 256, 64, 32, 4)
        assert c.n("conv_generic_fwd_window") == 1, c.d
        _check16(y2, k, layer, dtype, "window-mode conv_fwd", "conv16_fwd")
        # the pair form: one 64-wide K-step covers kernel rows (2t, 2t + 1), 4 steps two image rows apart; the eighth
        # kernel row and the eighth column are zero weights (n = 4 * 64 terms)
        wpair = torch.zeros(K, 8, 8, 4, dtype=dtype, device=DEV)
        wpair[:, :7, :7, :3] = k["wk"]
        wpair = wpair.reshape(K, 4 * 64).contiguous()
        kp = dict(k, n=4 * 64)
        for bm, bn in ((256, 64), (128, 64)):
            y3 = _nan(N, P, Q, K, dtype=dtype)
            with _Counts() as c:
                C.conv_fwd(xp, wpair, y3.view(-1), None, None, N, Hp, Wp, 64, K, 4, 1, P, Q, 2, 2, 0, 0, 2, 0, P, Q, 1, 1,
                           0, 0, bm, bn, 64, 4)
            assert c.n("conv_generic_fwd_window") == 1, c.d
            _check16(y3, kp, layer, dtype, f"window-pair conv_fwd tile {(bm, bn)}", "conv16_fwd")


# ============================================================================ the 3-channel first conv (VGG, AlexNet)
def _first_case(case, dtype, layer):
    """Operands, the padded NHWC4 image as VGGExecutor._forward sizes it, the production index maps
    (executor_vgg.first_conv_maps) and the fp64 references from the 16-bit image stem_pack stores."""
    from pytorch_distributed_template_amd.models.executor_vgg import first_conv_maps

    def make():
        C = _C()
        R, st, pad, N, H, W = case
        P, Q = cc.out_hw(cc.first_conv_geom(case))
        x, wk, dy = (_dev(t) for t in cc.first_conv_operands(case, dtype, layer))
        win, gidx, T, U, ldw = first_conv_maps(64, R)
        Hp, Wp = max(H + 2 * pad, (P - 1) * st + 2 * T), max(W + 2 * pad, (Q - 1) * st + 8 * U)
        xp = _nan(N * Hp * Wp * 4, dtype=dtype)
        C.stem_pack(x, xp, N, 3, H, W, pad, Hp, Wp)
        wwin = _nan(64 * R * U * 32, dtype=dtype)
        C.gather16(wk.reshape(-1), _dev(win), wwin)
        xr = x.to(dtype).permute(0, 2, 3, 1).contiguous()  # what stem_pack stores (round to nearest even)
        ref, mag = nm.conv_fwd_ref(xr, wk, st, pad)
        wref, wmag = nm.conv_wgrad_ref(xr, dy, R, R, st, pad)
        return dict(xp=xp, wwin=wwin, dy=dy, gidx=_dev(gidx), geom=(R, st, N, P, Q, Hp, Wp, T, U, ldw),
                    fwd=dict(ref=ref, mag=mag, n=R * U * 32), wg=dict(ref=wref, mag=wmag, n=N * P * Q))
    return _cached(("first", case, dtype, layer), make)


@pytest.mark.parametrize("layer", LAYERS)
@pytest.mark.parametrize("dtype", cc.DTYPES)
@pytest.mark.parametrize("stats", [False, True])
@pytest.mark.parametrize("case", cc.FIRST_CONV)
def test_first_conv_forward_window_mode(case, stats, dtype, layer):
    """Window-mode conv_fwd as VGGExecutor._forward calls it: one kernel row per tap row, U 8-pixel windows 8 pixels apart
    (U = 2: the 11- and 9-wide rows), tile (256, 64, 32), with and without the statistics slots.  The reduction holds
    R * U * 32 terms (the zero padding of the windows included): n of the bound."""
    C = _C()
    k = _first_case(case, dtype, layer)
    R, st, N, P, Q, Hp, Wp, T, U, ldw = k["geom"]
    y, sl = _nan(N, P, Q, 64, dtype=dtype), (_slots(C, 64) if stats else None)
    with _Counts() as c:
        C.conv_fwd(k["xp"], k["wwin"], y.view(-1), None, sl, N, Hp, Wp, 32, 64, R, U, P, Q, st, st, 0, 0, 1, 8, P, Q, 1, 1,
                   0, 0, 256, 64, 32, 4)
    assert c.n("conv_generic_fwd_window") == 1, c.d
    _check16(y, k["fwd"], layer, dtype, f"first conv {case} fwd", "conv16_fwd")
    if stats:
        _check_stats(sl.view(-1, 64, 2).sum(0), y, k["fwd"], layer, dtype, f"first conv {case} fwd")


@pytest.mark.parametrize("layer", LAYERS)
@pytest.mark.parametrize("dtype", cc.DTYPES)
@pytest.mark.parametrize("target", cc.WGRAD_TARGETS)
@pytest.mark.parametrize("case", cc.FIRST_CONV)
def test_first_conv_wgrad_window_mode(case, target, dtype, layer):
    """Window-mode conv_wgrad as VGGExecutor._first_wgrad calls it: T kernel-row pairs 2 rows apart x U 8-pixel windows
    8 pixels apart, then wgrad_reduce, then the production gather to KRSC.  The kernel's partials (summed in fp64) and
    the reducer's output are judged separately; the partials of the padding kernel row of an odd R and of the columns
    past R are finite, and the gather drops them."""
    C = _C()
    k = _first_case(case, dtype, layer)
    R, st, N, P, Q, Hp, Wp, T, U, ldw = k["geom"]
    splits, pps, _ = C.conv_wgrad_plan(64, T, U, 64, N * P * Q, target, True)
    ws = _nan(splits * 64 * ldw, dtype=torch.float32)
    with _Counts() as c:
        C.conv_wgrad(k["xp"], k["dy"], ws, N, Hp, Wp, 64, 64, T, U, P, Q, st, st, 0, 0, 2, 8, ldw, splits, pps, 4, True)
    assert c.n("conv_wgrad_window") == 1, c.d
    assert bool(torch.isfinite(ws).all()), "a partial (padding row / columns included) is not finite or was not written"
    name = f"first conv {case} wgrad target {target} ({splits} splits)"
    part = ws.view(splits, -1).double().sum(0)[k["gidx"].long()].view(64, R, R, 3)
    if layer == "int":
        nm.assert_exact(part, k["wg"]["ref"].float().double(), f"{name}: partials")
    else:
        _rec("conv16_wgrad", dtype, nm.assert_conv(part, k["wg"]["ref"], k["wg"]["mag"], k["wg"]["n"], torch.float32,
                                                   f"{name}: partials", "conv16_wgrad"))
    tmp = _nan(64 * ldw, dtype=torch.float32)
    C.wgrad_reduce(ws, splits, 64, ldw, ldw, 64 * ldw, tmp, ldw, 1.0, False)
    assert bool(torch.isfinite(tmp).all())
    dw = _nan(64 * R * R * 3, dtype=torch.float32)
    C.gather32(tmp, k["gidx"], dw)
    _check_wgrad(dw.view(64, R, R, 3), k["wg"], layer, name, dtype)


# ============================================================================ ResNet stem weight gradient, (T, U) = (4, 1)
def _stem_wgrad_case(nhw, dtype, layer):
    """The padded image, the tail operands with an argmax consistent with y, the independent fp64 dY
    (cc.stem_tail_ref) and the references of the plain (16-bit dY operand) and the fused weight gradient."""
    from pytorch_distributed_template_amd.models.executor_vgg import first_conv_maps

    def make():
        C = _C()
        N, H, W = nhw
        P, Q = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        d = {k: _dev(v) for k, v in cc.stem_fused_operands(N, H, W, dtype, layer).items()}
        r = cc.stem_tail_ref(d, N, P, Q, 64)
        _, gidx, T, U, ldw = first_conv_maps(64, 7)
        assert (T, U, ldw) == (4, 1, 256)
        Hp, Wp = max(H + 6, 2 * (P - 1) + 8), max(W + 6, 2 * (Q - 1) + 8)
        xp = _nan(N * Hp * Wp * 4, dtype=dtype)
        C.stem_pack(d["x"], xp, N, 3, H, W, 3, Hp, Wp)
        xr = d["x"].to(dtype).permute(0, 2, 3, 1).contiguous()
        n = N * P * Q
        # plain kernel: dY is an operand -- the reference dY rounded to the dtype (integer layer: unchanged)
        dy16 = r["dy"].float().to(dtype)
        pref, pmag = nm.conv_wgrad_ref(xr, dy16, 7, 7, 2, 3)
        fref, fmag = nm.conv_wgrad_ref(xr, r["dy"], 7, 7, 2, 3)
        if layer == "int":  # dY representable, every partial sum (in units of 1/2) below 2**24
            assert bool((nm.round_exact(r["dy"], dtype) == r["dy"]).all()) and 2 * float(fmag.max()) < 2.0 ** 24
            fbound = None
        else:
            fbound = nm.stem_fused_bound(xr, r["dy"], r["dymag"], n, dtype)
        return dict(d=d, xp=xp, dy16=dy16, gidx=_dev(gidx), geom=(N, P, Q, Hp, Wp), plain=dict(ref=pref, mag=pmag, n=n),
                    fref=fref, fbound=fbound)
    return _cached(("stem_wgrad", nhw, dtype, layer), make)


def _stem_plans(total):
    """Split plans over ``total`` (quad-padded) pixels: one split, the planner's for many blocks, 384-pixel splits (a
    ragged last one wherever total is no multiple of 384)."""
    splits, pps, _ = _C().conv_wgrad_plan(64, 4, 1, 64, total, 2048, True)
    if splits * pps < total:
        pps = (-(-total // splits) + 127) // 128 * 128
    return sorted({(1, (total + 127) // 128 * 128), (splits, pps), (-(-total // 384), 384)})


def _stem_judge(ws, splits, k, layer, dtype, name, fused):
    """The partials (fp64 sum) and wgrad_reduce's output, each gathered to KRSC through the production map."""
    C = _C()
    assert bool(torch.isfinite(ws).all()), f"{name}: a partial is not finite or was not written"
    tmp = _nan(64 * 256, dtype=torch.float32)
    C.wgrad_reduce(ws, splits, 64, 256, 256, 64 * 256, tmp, 256, 1.0, False)
    dw = _nan(64 * 7 * 7 * 3, dtype=torch.float32)
    C.gather32(tmp, k["gidx"], dw)
    part = ws.view(splits, -1).double().sum(0)[k["gidx"].long()]
    for what, got in (("partials", part), ("reduced", dw)):
        got = got.view(64, 7, 7, 3)
        if not fused:
            _check_wgrad(got.float(), k["plain"], layer, f"{name}: {what}", dtype)
        elif layer == "int":
            nm.assert_exact(got, k["fref"].float().double(), f"{name}: {what}")
        else:
            _rec("conv16_stem_fused", dtype, nm.assert_within(got, k["fref"], k["fbound"], f"{name}: {what}", 3,
                                                              "conv16_stem_fused", k["fref"].shape))


@pytest.mark.parametrize("layer", LAYERS)
@pytest.mark.parametrize("dtype", cc.DTYPES)
@pytest.mark.parametrize("nhw", cc.STEM_WGRAD_PLAIN)
def test_stem_wgrad_plain(nhw, dtype, layer):
    """wgrad_stem: the 7x7/2 weight gradient over the padded NHWC4 image with dY as a 16-bit operand, every split plan."""
    C = _C()
    k = _stem_wgrad_case(nhw, dtype, layer)
    N, P, Q, Hp, Wp = k["geom"]
    for splits, pps in _stem_plans(N * P * Q):
        ws = _nan(splits * 64 * 256, dtype=torch.float32)
        with _Counts() as c:
            C.conv_wgrad(k["xp"], k["dy16"], ws, N, Hp, Wp, 64, 64, 4, 1, P, Q, 2, 2, 0, 0, 2, 2, 256, splits, pps, 4, True)
        assert c.n("wgrad_stem") == 1 and c.n("wgrad_stem_fused") == 0, c.d
        _stem_judge(ws, splits, k, layer, dtype, f"wgrad_stem {nhw} ({splits} x {pps})", False)


@pytest.mark.parametrize("layer", LAYERS)
@pytest.mark.parametrize("dtype", cc.DTYPES)
@pytest.mark.parametrize("kernel,nhw", [("wgrad_stem_rows", g) for g in cc.STEM_WGRAD_ROWS] +
                         [("wgrad_stem_quad", g) for g in cc.STEM_WGRAD_QUAD])
def test_stem_wgrad_fused_dy_per_element(kernel, nhw, dtype, layer):
    """The fused stem weight gradients (dY = A*dz + B*y + C formed per 2x2 quad in the kernel and rounded to 16 bits before
    the MFMA) against the independent fp64 dY of cc.stem_tail_ref -- never against the two-pass path: ``int`` bit-exact,
    ``real`` within nm.stem_fused_bound.  The raw-row kernel needs a conv output of 4k x 16k pixels, every other shape
    runs the quad kernel (an odd height: half-dead last quads)."""
    C = _C()
    k = _stem_wgrad_case(nhw, dtype, layer)
    d = k["d"]
    N, P, Q, Hp, Wp = k["geom"]
    assert (P % 4 == 0 and Q % 16 == 0) == (kernel == "wgrad_stem_rows")
    for splits, pps in _stem_plans(N * ((P + 1) // 2) * 2 * Q):
        ws = _nan(splits * 64 * 256, dtype=torch.float32)
        with _Counts() as c:
            C.conv_wgrad_stem_fused(k["xp"], d["dp"], d["idx"], d["y"], d["coef"], d["b"], ws, N, Hp, Wp, 4, P, Q, 2, 2, 256,
                                    splits, pps)
        assert c.n("wgrad_stem_fused") == 1 and c.n("wgrad_stem_rows") == (1 if kernel == "wgrad_stem_rows" else 0), c.d
        _stem_judge(ws, splits, k, layer, dtype, f"{kernel} {nhw} ({splits} x {pps})", True)


# ============================================================================ weight gradients
def _wgrad_route(g, target, dtype, layer, plan_tile, counter):
    N, H, W, Ci, K, R, st, pad = g
    P, Q = cc.out_hw(g)
    assert _C().conv_wgrad_plan(K, R, R, Ci, N * P * Q, target, False)[2] == plan_tile
    k = _wgrad_case(g, dtype, layer)
    with _Counts() as c:
        dw, _ = _run_wgrad(k["x"], k["dy"], R, st, pad, target)
    assert c.n(counter) == 1, (counter, c.d)
    _check_wgrad(dw, k, layer, f"wgrad {g} target {target}", dtype)


@pytest.mark.parametrize("layer", LAYERS)
@pytest.mark.parametrize("dtype", cc.DTYPES)
@pytest.mark.parametrize("target", cc.WGRAD_TARGETS)
@pytest.mark.parametrize("g", cc.WGRAD_GENERIC)
def test_wgrad_generic_64x64(g, target, dtype, layer):
    _wgrad_route(g, target, dtype, layer, 64, "conv_wgrad_generic")


def _tile_counter(tile, g):
    """The counter of the kernel the planner's tile names."""
    if tile == 256:
        return "conv_wgrad_pp"
    if tile == 2:
        return "conv_wgrad_wide" if cc.out_hw(g)[1] >= 4 else "conv_wgrad_generic"
    if tile == 128:
        return "conv_wgrad_128_pair" if g[3] == 64 else "conv_wgrad_128"
    return "conv_wgrad_generic"


@pytest.mark.parametrize("layer", LAYERS)
@pytest.mark.parametrize("dtype", cc.DTYPES)
@pytest.mark.parametrize("target", cc.WGRAD_TARGETS)
@pytest.mark.parametrize("g", cc.WGRAD_ALEXNET)
def test_wgrad_alexnet_shapes_on_the_planners_tile(g, target, dtype, layer):
    N, H, W, Ci, K, R, st, pad = g
    P, Q = cc.out_hw(g)
    tile = _C().conv_wgrad_plan(K, R, R, Ci, N * P * Q, target, False)[2]
    _wgrad_route(g, target, dtype, layer, tile, _tile_counter(tile, g))


@pytest.mark.parametrize("layer", LAYERS)
@pytest.mark.parametrize("dtype", cc.DTYPES)
@pytest.mark.parametrize("target", cc.WGRAD_TARGETS)
@pytest.mark.parametrize("g", cc.WGRAD_CLASSIFIER)
def test_wgrad_classifier_with_cropped_reduce(g, target, dtype, layer):
    """The classifier's weight gradient: a 1x1 conv over H = W = 1 (5 and 130 pixels in all), then wgrad_reduce over
    rows = cout - 28 with ldo = cols: the rows it owns hold the gradient, the rows beyond stay untouched (NaN)."""
    C = _C()
    N, H, W, Ci, K, R, st, pad = g
    k = _wgrad_case(g, dtype, layer)
    splits, pps, tile = C.conv_wgrad_plan(K, 1, 1, Ci, N, target, False)
    ws = _nan(splits * K * Ci, dtype=torch.float32)
    with _Counts() as c:
        C.conv_wgrad(k["x"], k["dy"], ws, N, 1, 1, Ci, K, 1, 1, 1, 1, 1, 1, 0, 0, 1, 1, Ci, splits, pps, 0, False)
    assert c.n(_tile_counter(tile, g)) == 1, c.d
    name = f"classifier wgrad {g} target {target} ({splits} splits)"
    part = dict(k, ref=k["ref"].view(K, Ci), mag=k["mag"].view(K, Ci))
    _check_wgrad(ws.view(splits, K, Ci).double().sum(0).float(), part, layer, f"{name}: partials", dtype)
    rows = K - 28
    out = _nan(K, Ci, dtype=torch.float32)
    C.wgrad_reduce(ws, splits, rows, Ci, Ci, K * Ci, out, Ci, 1.0, False)
    crop = dict(k, ref=k["ref"].view(K, Ci)[:rows], mag=k["mag"].view(K, Ci)[:rows])
    _check_wgrad(out[:rows], crop, layer, name, dtype)
    assert bool(torch.isnan(out[rows:]).all()), f"{name}: wgrad_reduce wrote beyond its rows"


@pytest.mark.parametrize("layer", LAYERS)
@pytest.mark.parametrize("dtype", cc.DTYPES)
@pytest.mark.parametrize("target", cc.WGRAD_TARGETS)
@pytest.mark.parametrize("g", cc.WGRAD_PAIR)
def test_wgrad_two_tap_pair_tile(g, target, dtype, layer):
    # a 3-wide output runs the pair tile's split plan on the 64 x 64 kernel (conv_wgrad_launch)
    _wgrad_route(g, target, dtype, layer, 128, "conv_wgrad_128_pair" if cc.out_hw(g)[1] >= 4 else "conv_wgrad_generic")


@pytest.mark.parametrize("layer", LAYERS)
@pytest.mark.parametrize("dtype", cc.DTYPES)
@pytest.mark.parametrize("target", cc.WGRAD_TARGETS)
@pytest.mark.parametrize("g", cc.WGRAD_WIDE)
def test_wgrad_wide_256x128(g, target, dtype, layer):
    _wgrad_route(g, target, dtype, layer, 2, "conv_wgrad_wide" if cc.out_hw(g)[1] >= 4 else "conv_wgrad_generic")


@pytest.mark.parametrize("layer", LAYERS)
@pytest.mark.parametrize("dtype", cc.DTYPES)
@pytest.mark.parametrize("target", [64, 1024])
@pytest.mark.parametrize("g", cc.WGRAD_PP)
def test_wgrad_pingpong_256(g, target, dtype, layer):
    _wgrad_route(g, target, dtype, layer, 256, "conv_wgrad_pp")


@pytest.mark.parametrize("layer", LAYERS)
@pytest.mark.parametrize("dtype", cc.DTYPES)
@pytest.mark.parametrize("fused", [False, True])
def test_wgrad_3x3c64_all_taps(fused, dtype, layer):
    """The layer1 weight-gradient kernel (partial last row tile), plain and over the producer's raw output with its
    BN + ReLU applied to the staged tiles."""
    C = _C()
    N, H, W = cc.WGRAD_L1 if not fused else (3, 12, 56)
    g = (N, H, W, 64, 64, 3, 1, 1)

    def make():
        x, dy = cc.wgrad_operands(g, dtype, layer)
        x, dy = _dev(x), _dev(dy)
        coef = _dev(cc.pre_operands(layer, dtype)) if fused else None
        a = cc.pre_apply_ref(x, coef, dtype).float().to(dtype) if fused else x
        ref, mag = nm.conv_wgrad_ref(a, dy, 3, 3, 1, 1)
        return dict(x=x, dy=dy, coef=coef, ref=ref, mag=mag, n=N * H * W)
    k = _cached(("wgrad_l1", g, fused, dtype, layer), make)
    blocks = C.wgrad_blocks_3x3c64()
    ws = _nan(blocks * 64 * 576, dtype=torch.float32)
    if fused:
        parts = C.conv_wgrad_3x3c64(k["x"], k["dy"], ws, N, H, W, k["coef"])
    else:
        parts = C.conv_wgrad_3x3c64(k["x"], k["dy"], ws, N, H, W)
    out = _nan(64 * 576, dtype=torch.float32)
    C.wgrad_reduce(ws, parts, 64, 576, 576, 64 * 576, out, 576, 1.0, False)
    _check_wgrad(out.view(64, 3, 3, 64), k, layer, f"conv_wgrad_3x3c64 fused={fused}", dtype)


@pytest.mark.parametrize("layer", LAYERS)
@pytest.mark.parametrize("dtype", cc.DTYPES)
def test_wgrad_pair_tile_fused_producer_bn_relu(dtype, layer):
    """1x1 64 -> 256 weight gradient over the producer's raw output (M = 12581: a 37-row tail whose zero-filled rows
    transform to relu(shift) and must meet zero dY rows)."""
    C = _C()
    M = 12544 + 37
    g = cc.c64_geom(M)

    def make():
        x, dy = cc.wgrad_operands(g, dtype, layer)
        x, dy = _dev(x), _dev(dy)
        coef = _dev(cc.pre_operands(layer, dtype))
        a = cc.pre_apply_ref(x, coef, dtype).float().to(dtype)
        ref, mag = nm.conv_wgrad_ref(a, dy, 1, 1, 1, 0)
        return dict(x=x, dy=dy, coef=coef, ref=ref, mag=mag, n=M)
    k = _cached(("wgrad_pair_pre", g, dtype, layer), make)
    with _Counts() as c:
        dw, tile = _run_wgrad(k["x"], k["dy"], 1, 1, 0, 512, pre=k["coef"])
    assert tile == 128 and c.n("conv_wgrad_128_pair_fused_bn_relu") == 1, c.d
    _check_wgrad(dw, k, layer, "wgrad pair tile + producer BN", dtype)
