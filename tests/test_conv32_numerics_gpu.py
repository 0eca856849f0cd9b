"""Every fp32 MFMA conv route (csrc/kernels/fp32.hip) per element against an independent fp64 reference (MI355X).

Three layers per route (tests/_numerics.py derives the bounds, tests/_conv_cases.py holds the cases and the operands,
tests/test_numerics_model_cpu.py proves that the assertions bite):

* ``int``: operands from {-2, -1, 1, 2} x {-1, 1} and the exact BN operands.  Every product and partial sum is an
  integer below 2**24, so outputs, statistics and fused BN-backward sums must EQUAL the fp64 reference in any order,
  grouping, split or tile walk: any mismatch is a dropped, doubled or misplaced term.
* ``real``: randn operands, one output channel scaled by 1e-3; every element within ``(n + 5) * 2u * mag``: this layer
  owns scaling and rounding-mode errors.
* ``wide``: 1x1 geometries whose every output is exactly one non-zero product that needs all 24 bits of the multiply
  (or of one operand): bit-exact, so a product or an operand kept to fewer bits fails in every element.

No reference comes from a kernel of this project or from another GPU library: outputs are compared with ``F.unfold`` +
``matmul`` in float64 on the fp32 values the kernel reads, statistics with fp64 sums of the stored output, the fused
BN-backward sums with sums over the independent ``dz``, the stem's fused dY with an fp64 scatter along the argmax bytes.
Outputs and workspaces are pre-filled with NaN and every test asserts through the dispatch counters that the route it
names ran.  A split that owns no pixel is produced by no caller and is not run.
"""
import pytest
import torch

import _conv_cases as cc
import _numerics as nm

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32 = torch.float32
LAYERS = ["int", "real"]

_cache = {}


def _cached(key, make):
    if key not in _cache:
        if len(_cache) > 8:
            _cache.pop(next(iter(_cache)))
        _cache[key] = make()
    return _cache[key]


def _dev(t):
    return None if t is None else t.to(DEV).contiguous()


def _C():
    from pytorch_distributed_template_amd.ops import native
    return native.C


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=F32, device=DEV)


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


@pytest.fixture
def halo_setting():
    """conv32_set_halo restored after the test."""
    prev = _C().conv32_set_halo(1)
    yield _C().conv32_set_halo
    _C().conv32_set_halo(prev)


# ------------------------------------------------------------------------------------------------ cases (cached)
def _fwd_case(g, layer):
    def make():
        x, w, res = (_dev(t) for t in cc.fwd_operands(g, F32, layer, residual=True))
        plain = nm.conv_fwd_ref(x, w, g[6], g[7])
        withres = nm.conv_fwd_ref(x, w, g[6], g[7], res)
        return dict(x=x, w=w, res=res, ref={False: plain[0], True: withres[0]}, mag={False: plain[1], True: withres[1]},
                    n=g[3] * g[5] * g[5])
    return _cached(("fwd", g, layer), make)


def _dgrad_case(g, layer):
    def make():
        dy, w, res = (_dev(t) for t in cc.dgrad_operands(g, F32, layer, "full"))
        plain = nm.conv_dgrad_ref(dy, w, g[1], g[2], g[6], g[7])
        withres = nm.conv_dgrad_ref(dy, w, g[1], g[2], g[6], g[7], res)
        wt, phases = _phase_weights(w, g[6], g[7], g[1], g[2])
        return dict(dy=dy, w=w, wt=wt, phases=phases, res=res, ref={False: plain[0], True: withres[0]},
                    mag={False: plain[1], True: withres[1]}, n=g[4] * g[5] * g[5])
    return _cached(("dgrad", g, layer), make)


def _wgrad_case(g, layer):
    def make():
        x, dy = (_dev(t) for t in cc.wgrad_operands(g, F32, layer))
        ref, mag = nm.conv_wgrad_ref(x, dy, g[5], g[5], g[6], g[7])
        P, Q = cc.out_hw(g)
        return dict(x=x, dy=dy, ref=ref, mag=mag, n=g[0] * P * Q)
    return _cached(("wgrad", g, layer), make)


def _phase_weights(w, stride, pad, H, W):
    """(phase weights Wt[c][t][u][k] of every sub-pixel phase, concatenated; the phase table of conv32_dgrad)."""
    from pytorch_distributed_template_amd.ops import conv
    K, R, S, Ci = w.shape
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
    return torch.cat(pieces).contiguous(), phases


# ----------------------------------------------------------------------------------------------------- checks
def _check(out, ref, mag, n, layer, name, family, K=None):
    assert out.shape == ref.shape, f"{name}: shape {tuple(out.shape)} vs {tuple(ref.shape)}"
    if layer == "real":
        return nm.assert_conv32(out, ref, mag, n, name, family)
    top, sumsq = nm.int32_case_conditions(ref, mag, K or ref.shape[-1])
    assert top < 2.0 ** 24 and sumsq < 2.0 ** 24, f"{name}: not an exact case ({top}, {sumsq})"
    nm.assert_exact(out, ref, name)
    assert torch.equal(out.double(), ref)


def _check_stats(sp, y, K, layer, name):
    sums = sp.view(-1, K, 2).sum(0)
    nm.assert_conv_stats(sums[:, 0], sums[:, 1], y, name, family="conv32_stats", exact=layer == "int")


def _run_fwd(k, g, tile, variant, name, layer, counter="conv32_fwd", halo=None):
    C = _C()
    N, H, W, Ci, K, R, st, pad = g
    P, Q = cc.out_hw(g)
    res = "res" in variant
    stats = "stats" in variant
    y = _nan(N, P, Q, K)
    sp = _slots(C, K) if stats else None
    with _Counts() as c:
        C.conv32_fwd(k["x"], k["w"].reshape(-1), y, k["res"] if res else None, sp, N, H, W, Ci, K, R, R, P, Q, st, pad,
                     *tile)
    assert c.n(counter) == 1 and c.n("conv32_dgrad") == 0, c.d
    if halo is not None:
        assert c.n("conv32_halo") == halo, (name, c.d)
    _check(y, k["ref"][res], k["mag"][res], k["n"], layer, name, "conv32_fwd")
    if stats:
        _check_stats(sp, y, K, layer, name)


def _run_dgrad(k, g, tile, epi, layer, name, halo=None):
    """One conv32_dgrad launch with the epilogue ``epi`` of cc.C32_EPILOGUES, checked per element and per sum."""
    C = _C()
    ename, mode, res = epi
    N, H, W, Ci, K, R, st, pad = g
    P, Q = cc.out_hw(g)
    dx = _nan(N, H, W, Ci)
    kw = {}
    if mode:
        d = {key: _dev(v) for key, v in cc.bnb_operands(mode, (N, H, W, Ci), F32, layer).items()}
        slots = _slots(C, Ci, 4 if mode == 3 else 2)
        kw = dict(bn_mref=d["out"], bn_y1=d["y1"], bn_coef=d["coef1"], stats=slots, bn_y2=d["y2"], bn_coef2=d["coef2"])
    with _Counts() as c:
        C.conv32_dgrad(k["dy"], k["wt"], dx, k["res"] if res else None, N, P, Q, K, Ci, H, W, st, k["phases"], *tile,
                       **kw)
    assert c.n("conv32_dgrad") == 1 and c.n("conv32_fwd") == 0, c.d
    assert c.n("conv32_dgrad_bn_reduce_epilogue") == (1 if mode else 0), c.d
    if halo is not None:
        assert c.n("conv32_halo") == halo, (name, c.d)
    ref, mag = k["ref"][res], k["mag"][res]
    if not mode:
        _check(dx, ref, mag, k["n"], layer, name, "conv32_dgrad")
        return
    _check_bnb(mode, dx, slots, ref, mag, k["n"], d, layer, name)


def _check_bnb(mode, dz, slots, ref, mag, n, d, layer, name):
    """dz = dgrad_ref * mask per element, and sum dz, sum dz * xhat (both branches) against sums over that reference."""
    Cc = ref.shape[-1]
    KO = 4 if mode == 3 else 2
    sums = slots.view(-1, Cc, KO).sum(0)
    mask, unsure = cc.bnb_mask(mode, d, Cc)
    zero = torch.zeros((), dtype=torch.float64, device=DEV)
    mref = torch.where(mask, ref.reshape(-1, Cc), zero)
    x1 = nm.bn_xhat(d["y1"], d["coef1"], Cc)
    x2 = nm.bn_xhat(d["y2"], d["coef2"], Cc) if mode == 3 else None
    if layer == "int":
        assert not bool(unsure.any())
        assert float(mag.max()) < 2.0 ** 24
        for xh in (x1, x2)[:2 if mode == 3 else 1]:  # sums in quarters (invstd >= 0.25): exact below 2**22
            assert float((mref * xh).abs().sum(0).max()) < 2.0 ** 22, name
        nm.assert_exact(dz.reshape(-1, Cc), mref, f"{name}: dz")
        nm.assert_bnb_sums(sums[:, 0], sums[:, 1], mref, None, x1, f"{name}: branch 1", exact=True)
        if mode == 3:
            nm.assert_bnb_sums(sums[:, 2], sums[:, 3], mref, None, x2, f"{name}: branch 2", exact=True)
        return
    full = nm.conv32_bound(mag, n).reshape(-1, Cc)
    bound = torch.where(mask, full, torch.zeros_like(full))
    share = float(unsure.double().mean().item())
    assert share < 0.01, f"{name}: {share:.5f} of the pre-activations are too close to zero to call"
    # elements whose ReLU sign fp32 may call either way: left out of the element comparison, and either value (0 or
    # the data gradient) is accepted inside the sums
    got = torch.where(unsure, mref, dz.reshape(-1, Cc).double())
    nm.assert_within(got, mref, bound, f"{name}: dz", Cc, "conv32_dgrad", mref.shape)
    sb = torch.where(unsure, ref.reshape(-1, Cc).abs() + full, bound)
    nm.assert_bnb_sums(sums[:, 0], sums[:, 1], mref, sb, x1, f"{name}: branch 1", family="conv32_bnb_sums")
    if mode == 3:
        nm.assert_bnb_sums(sums[:, 2], sums[:, 3], mref, sb, x2, f"{name}: branch 2", family="conv32_bnb_sums")


# ============================================================================ every tile of conv32_kernel
@pytest.mark.parametrize("layer", LAYERS)
@pytest.mark.parametrize("tile", cc.C32_TILES)
def test_every_tile_forward_every_variant(tile, layer, halo_setting):
    """Strided 3x3, 13 x 13 x 11, 128 -> 256 (546 rows: ragged on 128, 256 and 512) on every compiled tile: plain,
    residual, statistics, statistics + residual."""
    g = cc.C32_TILE_GEOM
    k = _fwd_case(g, layer)
    for variant in cc.C32_FWD_VARIANTS:
        _run_fwd(k, g, tile, variant, f"fwd tile {tile} {variant}", layer, halo=0)


@pytest.mark.parametrize("layer", LAYERS)
@pytest.mark.parametrize("epi", cc.C32_EPILOGUES, ids=lambda e: e[0])
@pytest.mark.parametrize("tile", cc.C32_TILES)
def test_every_tile_backward_data_every_epilogue(tile, epi, layer, halo_setting):
    """Four phases of 546 / 455 / 468 / 390 rows (2/1/1/1 tiles of 512 rows, 3/2/2/2 of 256, 5/4/4/4 of 128): the grid is
    sized for the largest phase, the surplus blocks must zero the statistics rows they own."""
    g = cc.C32_TILE_GEOM_256 if tile[1] == 256 else cc.C32_TILE_GEOM
    k = _dgrad_case(g, layer)
    assert len(k["phases"]) == 4
    _run_dgrad(k, g, tile, epi, layer, f"dgrad tile {tile} {epi[0]}", halo=0)


# ============================================================================ the executor's default tiles
@pytest.mark.parametrize("layer", LAYERS)
@pytest.mark.parametrize("g", cc.C32_DEFAULT_GEOMS, ids=str)
def test_default_tile_forward(g, layer, halo_setting):
    P, Q = cc.out_hw(g)
    tile = cc.tile32_default(g[4], g[0] * P * Q)
    halo_setting(0)  # conv32_kernel: the halo kernel has its own tests
    k = _fwd_case(g, layer)
    for variant in ("stats_res", "plain"):
        _run_fwd(k, g, tile, variant, f"fwd {g} {tile} {variant}", layer, halo=0)


@pytest.mark.parametrize("layer", LAYERS)
@pytest.mark.parametrize("g", cc.dgrad_geoms32_default(), ids=str)
def test_default_tile_backward_data(g, layer, halo_setting):
    P, Q = cc.out_hw(g)
    tile = cc.tile32_default(g[3], g[0] * P * Q)
    halo_setting(0)
    k = _dgrad_case(g, layer)
    if g[5] == 1 and g[6] == 2:  # three phases without taps hold the residual alone
        assert len(k["phases"]) == 4 and sum(1 for p in k["phases"] if p[2] == 0 or p[3] == 0) == 3
    for epi in (cc.C32_EPILOGUES[1], cc.C32_EPILOGUES[3], cc.C32_EPILOGUES[5]):
        _run_dgrad(k, g, tile, epi, layer, f"dgrad {g} {tile} {epi[0]}", halo=0)


# ============================================================================ conv32_halo_kernel
@pytest.mark.parametrize("layer", LAYERS)
@pytest.mark.parametrize("halo", [1, 0])
@pytest.mark.parametrize("g", cc.C32_HALO_GEOMS, ids=str)
def test_halo_kernel_every_variant_and_the_restaging_kernel(g, halo, layer, halo_setting):
    """3x3/s1/p1, bn = 64: forward (EPI 0, 1 x RES) and single-phase backward data (EPI 0, 2, 3 x RES and the mask
    recomputed from y1) on the halo kernel and, with the halo kernel off, on conv32_kernel -- the same expectation."""
    halo_setting(halo)
    k = _fwd_case(g, layer)
    for variant in cc.C32_FWD_VARIANTS:
        _run_fwd(k, g, (128, 64), variant, f"halo={halo} fwd {g} {variant}", layer, halo=halo)
    gd = cc.dgrad_geom32(g)
    kd = _dgrad_case(gd, layer)
    assert len(kd["phases"]) == 1
    for epi in cc.C32_EPILOGUES:
        _run_dgrad(kd, gd, (128, 64), epi, layer, f"halo={halo} dgrad {gd} {epi[0]}", halo=halo)


@pytest.mark.parametrize("layer", LAYERS)
@pytest.mark.parametrize("g", cc.C32_HALO_REFUSED, ids=str)
def test_halo_kernel_refuses_the_neighbouring_widths(g, layer, halo_setting):
    """W = 57 and W = 2 need more than 464 LDS rows: with the halo kernel on, conv32_kernel runs and is right."""
    halo_setting(1)
    k = _fwd_case(g, layer)
    _run_fwd(k, g, (128, 64), "stats_res", f"refused fwd {g}", layer, halo=0)
    gd = cc.dgrad_geom32(g)
    kd = _dgrad_case(gd, layer)
    for epi in (cc.C32_EPILOGUES[1], cc.C32_EPILOGUES[5]):
        _run_dgrad(kd, gd, (128, 64), epi, layer, f"refused dgrad {gd} {epi[0]}", halo=0)


# ============================================================================ weight gradients
def _check_wgrad(ws, dw, splits, k, layer, name):
    """The kernel (fp64 sum of its split partials) and the reducer (wgrad_reduce's fp32 sum) judged separately."""
    ref, mag = k["ref"], k["mag"]
    part = ws.view(splits, *ref.shape).double().sum(0)
    if layer == "int":
        assert float(mag.max()) < 2.0 ** 24
        nm.assert_exact(part, ref, f"{name}: partials")
        nm.assert_exact(dw.view(ref.shape), ref, f"{name}: reduced")
        return
    nm.assert_conv32(part, ref, mag, k["n"], f"{name}: partials", "conv32_wgrad")
    nm.assert_conv32(dw.view(ref.shape), ref, mag, k["n"], f"{name}: reduced", "conv32_wgrad")


def _run_wgrad(g, tile, layer, counter):
    C = _C()
    N, H, W, Ci, K, R, st, pad = g
    P, Q = cc.out_hw(g)
    k = _wgrad_case(g, layer)
    ldw = R * R * Ci
    plans = cc.wgrad32_plans(g, tile)
    assert plans[0][0] == 1
    for splits, pps in plans:
        ws = _nan(splits * K * ldw)
        with _Counts() as c:
            C.wgrad32(k["x"], k["dy"], ws, N, H, W, Ci, K, R, R, P, Q, st, pad, ldw, splits, pps, tile)
        assert c.n(counter) == 1 and sum(c.n(x) for x in ("wgrad32", "wgrad32_wide", "wgrad32_halo")) == 1, c.d
        dw = _nan(K * ldw)
        C.wgrad_reduce(ws, splits, K, ldw, ldw, K * ldw, dw, ldw, 1.0, False)
        _check_wgrad(ws, dw, splits, k, layer, f"wgrad32 tile {tile} {g} plan {(splits, pps)}")


@pytest.mark.parametrize("layer", LAYERS)
@pytest.mark.parametrize("g", cc.W32_T64, ids=str)
def test_wgrad32_tile_64(g, layer):
    _run_wgrad(g, 64, layer, "wgrad32")


@pytest.mark.parametrize("layer", LAYERS)
@pytest.mark.parametrize("g", cc.W32_T128, ids=str)
def test_wgrad32_tile_128(g, layer):
    _run_wgrad(g, 128, layer, "wgrad32_wide")


@pytest.mark.parametrize("layer", LAYERS)
@pytest.mark.parametrize("g", cc.W32_HALO, ids=str)
def test_wgrad32_halo_tile(g, layer):
    """Splits over output rows: one split, the executor's plan, a partial last split, one output row per split."""
    assert any(pps == 1 for _, pps in cc.wgrad32_plans(g, 3))
    _run_wgrad(g, 3, layer, "wgrad32_halo")


# ============================================================================ the width of the multiply
@pytest.mark.parametrize("variant", cc.WIDE_VARIANTS)
@pytest.mark.parametrize("g", cc.WIDE_FWD, ids=str)
def test_wide_forward_and_backward_data_are_single_products(g, variant, halo_setting):
    """Each output is one product of a 12 x 12-bit pair (a) or a 24-bit operand with +-{1, 2, 4} (b, c): bit-exact on
    every tile that fits."""
    C = _C()
    N, H, W, Ci, K, R, st, pad = g
    x, w = (_dev(t) for t in cc.wide_fwd_operands(g, variant))
    ref, _ = nm.conv_fwd_ref(x, w, 1, 0)
    assert bool((ref != 0).all()) and bool((ref.float().double() == ref).all())
    for tile in [t for t in cc.C32_TILES if K % t[1] == 0]:
        y = _nan(N, H, W, K)
        with _Counts() as c:
            C.conv32_fwd(x, w.reshape(-1), y, None, None, N, H, W, Ci, K, 1, 1, H, W, 1, 0, *tile)
        assert c.n("conv32_fwd") == 1, c.d
        nm.assert_exact(y, ref, f"wide {variant} fwd {g} tile {tile}")
    gd = cc.dgrad_geom32(g)  # dY has Ci channels (the reduction), dX has K
    dy, wd = (_dev(t) for t in cc.wide_dgrad_operands(gd, variant))
    refd, _ = nm.conv_dgrad_ref(dy, wd, H, W, 1, 0)
    assert bool((refd != 0).all())
    wt, phases = _phase_weights(wd, 1, 0, H, W)
    for tile in [t for t in cc.C32_TILES if K % t[1] == 0]:
        dx = _nan(N, H, W, K)
        with _Counts() as c:
            C.conv32_dgrad(dy, wt, dx, None, N, H, W, Ci, K, H, W, 1, phases, *tile)
        assert c.n("conv32_dgrad") == 1, c.d
        nm.assert_exact(dx, refd, f"wide {variant} dgrad {gd} tile {tile}")


@pytest.mark.parametrize("variant", cc.WIDE_VARIANTS)
@pytest.mark.parametrize("g,tile", cc.WIDE_WGRAD, ids=str)
def test_wide_weight_gradient_is_single_products(g, tile, variant):
    C = _C()
    N, H, W, Ci, K, R, st, pad = g
    x, dy = (_dev(t) for t in cc.wide_wgrad_operands(g, variant))
    ref, _ = nm.conv_wgrad_ref(x, dy, 1, 1, 1, 0)
    assert bool((ref != 0).all()) and bool((ref.float().double() == ref).all())
    for splits, pps in cc.wgrad32_plans(g, tile):
        ws = _nan(splits * K * Ci)
        with _Counts() as c:
            C.wgrad32(x, dy, ws, N, H, W, Ci, K, 1, 1, H, W, 1, 0, Ci, splits, pps, tile)
        assert c.n("wgrad32_wide" if tile == 128 else "wgrad32") == 1, c.d
        dw = _nan(K * Ci)
        C.wgrad_reduce(ws, splits, K, Ci, Ci, K * Ci, dw, Ci, 1.0, False)
        nm.assert_exact(ws.view(splits, K, 1, 1, Ci).double().sum(0), ref, f"wide {variant} wgrad {g}: partials")
        nm.assert_exact(dw.view(K, 1, 1, Ci), ref, f"wide {variant} wgrad {g}: reduced")


# ============================================================================ window-mode stem
def _stem_dims(H, W):
    P, Q = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    return P, Q, max(H + 6, (P - 1) * 2 + 8), max(W + 6, (Q - 1) * 2 + 8)


def _stem_case(N, H, W, layer):
    """The padded NHWC4 image is built with torch (stem_pack32 has its own test in test_bn_chain_gpu.py)."""
    def make():
        P, Q, Hp, Wp = _stem_dims(H, W)
        x, w, dy = (_dev(t) for t in cc.stem32_operands(N, H, W, layer))
        xh = x.permute(0, 2, 3, 1).contiguous()
        xp = torch.zeros(N, Hp, Wp, 4, device=DEV)
        xp[:, 3:3 + H, 3:3 + W, :3] = xh
        ww = torch.zeros(64, 7, 8, 4, device=DEV)
        ww[:, :, :7, :3] = w
        ref, mag = nm.conv_fwd_ref(xh, w, 2, 3)
        wref, wmag = nm.conv_wgrad_ref(xh, dy, 7, 7, 2, 3)
        return dict(xh=xh, xp=xp.reshape(-1), ww=ww.reshape(-1).contiguous(), dy=dy, ref=ref, mag=mag, wref=wref,
                    wmag=wmag)
    return _cached(("stem", N, H, W, layer), make)


def _stem_plans(npix):
    """One split, and five splits whose last one is partial (pix_per_split a multiple of 64)."""
    pps = ((npix + 4) // 5 + 63) // 64 * 64
    return sorted({(1, (npix + 63) // 64 * 64), (-(-npix // pps), pps)})


def _stem_dw(ws, splits):
    """ws[split][k][pair][row in pair][pixel s][channel] -> (dW [64, 7, 7, 3], the channel-3 entries)."""
    full = ws.view(splits, 64, 8, 8, 4).double().sum(0)
    return full[:, :7, :7, :3], full[..., 3]


@pytest.mark.parametrize("layer", LAYERS)
@pytest.mark.parametrize("tile", cc.STEM32_TILES)
@pytest.mark.parametrize("N,H,W", cc.STEM32)
def test_conv32_stem_forward_window_mode(N, H, W, tile, layer):
    """conv32 over the zero-padded NHWC4 image (K = 7 kernel rows x (8 pixels x 4 channels)) with statistics."""
    C = _C()
    P, Q, Hp, Wp = _stem_dims(H, W)
    k = _stem_case(N, H, W, layer)
    y, sp = _nan(N, P, Q, 64), _slots(C, 64)
    with _Counts() as c:
        C.conv32_stem_fwd(k["xp"], k["ww"], y.view(-1), sp, N, Hp, Wp, 7, P, Q, 2, 64, *tile)
    assert c.n("conv32_fwd") == 1 and c.n("conv32_halo") == 0, c.d
    name = f"conv32_stem_fwd {(N, H, W)} tile {tile}"
    _check(y, k["ref"], k["mag"], 7 * 32, layer, name, "conv32_fwd")
    _check_stats(sp, y, 64, layer, name)


@pytest.mark.parametrize("layer", LAYERS)
@pytest.mark.parametrize("all_pairs", [0, 1])
@pytest.mark.parametrize("N,H,W", cc.STEM32_FUSED)
def test_wgrad32_stem_window_pairs(N, H, W, all_pairs, layer):
    """One block per kernel-row pair (wgrad32_kernel) and all four pairs per block (wgrad32_stem4_kernel)."""
    C = _C()
    P, Q, Hp, Wp = _stem_dims(H, W)
    k = _stem_case(N, H, W, layer)
    npix = N * P * Q
    for splits, pps in _stem_plans(npix):
        ws = _nan(splits * 64 * 256)
        with _Counts() as c:
            C.wgrad32_stem(k["xp"], k["dy"], ws, N, Hp, Wp, 4, 64, P, Q, 2, splits, pps, all_pairs)
        assert c.n("wgrad32_stem4") == all_pairs and c.n("wgrad32") == 1 - all_pairs, c.d
        dw, ch3 = _stem_dw(ws, splits)
        assert bool((ch3 == 0).all()), "the padding channel of the NHWC4 image has a weight gradient"
        name = f"wgrad32_stem all_pairs={all_pairs} {(N, H, W)} plan {(splits, pps)}"
        if layer == "int":
            nm.assert_exact(dw, k["wref"], name)
        else:
            nm.assert_conv32(dw, k["wref"], k["wmag"], npix, name, "conv32_wgrad")


@pytest.mark.parametrize("layer", LAYERS)
@pytest.mark.parametrize("N,H,W", cc.STEM32_FUSED)
def test_wgrad32_stem_fused_dy_against_an_independent_fp64_dy(N, H, W, layer):
    """dY formed inside the kernel (max-pool backward along random argmax codes -- codes pointing outside the image
    included --, ReLU mask, A*dz + B*y + C) against the fp64 scatter of cc.stem_tail_ref followed by the fp64 weight
    gradient.  A pixel whose ReLU sign fp32 may call either way may contribute |A*dz| or nothing: that much joins the
    bound of the sums it enters."""
    C = _C()
    P, Q, Hp, Wp = _stem_dims(H, W)
    k = _stem_case(N, H, W, layer)
    npix = N * P * Q

    def make():
        d = {key: _dev(v) for key, v in cc.stem32_tail_operands(N, P, Q, layer).items()}
        r = cc.stem_tail_ref(d, N, P, Q, 64)
        ref, _ = nm.conv_wgrad_ref(k["xh"], r["dy"], 7, 7, 2, 3)
        _, mag = nm.conv_wgrad_ref(k["xh"], r["dymag"], 7, 7, 2, 3)
        _, flip = nm.conv_wgrad_ref(k["xh"], r["dyflip"], 7, 7, 2, 3)
        return d, r, ref, mag, flip
    d, r, ref, mag, flip = _cached(("stem_fused", N, H, W, layer), make)
    assert float(r["unsure"].double().mean()) < 0.01
    plans = _stem_plans(npix)
    if (N, H, W) == (3, 40, 36):  # the case with a partial last 32-pixel chunk and an odd pooled width
        assert npix % 32 != 0 and ((Q - 1) // 2 + 1) % 2 == 1
    for splits, pps in plans:
        ws = _nan(splits * 64 * 256)
        with _Counts() as c:
            C.wgrad32_stem_fused(k["xp"], d["dp"].view(-1), d["idx"].view(-1), d["y"].view(-1), d["coef"], d["b"], ws,
                                 N, Hp, Wp, P, Q, 2, splits, pps)
        assert c.n("wgrad32_stem4_fused") == 1 and c.n("wgrad32_stem4") == 0, c.d
        dw, ch3 = _stem_dw(ws, splits)
        assert bool((ch3 == 0).all())
        name = f"wgrad32_stem_fused {(N, H, W)} plan {(splits, pps)}"
        if layer == "int":
            assert not bool(r["unsure"].any()) and float(mag.max()) < 2.0 ** 23  # dY in halves: exact below 2**23
            nm.assert_exact(dw, ref, name)
        else:
            nm.assert_within(dw, ref, nm.conv32_bound(mag, npix, extra=12) + flip, name, 3, "conv32_stem_fused",
                             ref.shape)
