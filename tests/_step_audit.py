"""Teacher-forced audit of one ResNetExecutor step (a plain module, not a conftest).

``extract_record`` turns what a step left behind -- the executor's ``saved`` forward intermediates and the ``Tape`` of
its launches (tests/_tape.py) -- into a ``StepRecord``: plain named tensors in logical layout (NHWC activations,
``p.grad`` views), named after the ``nn.Module`` tree.  It is the only part that knows buffer keys and tape positions.

``audit`` walks the module tree and judges EVERY tensor of the record per element against an fp64 reference computed
from the record's own upstream tensors and the model's parameters in their logical torch layout
(``conv.weight.detach().to(dtype).double()``, ``bn.eps``, ``bn.momentum``, buffers snapshotted before the step): errors do
not compound, so the per-kernel bounds of tests/_numerics.py and tests/_pool_cases.py apply unchanged.  The reference
never reads the executor's shadow, derived layouts, index maps or helpers.  It runs on the device of the record (pure
torch fp64), so tests/test_step_audit_cpu.py proves it on emulated records.

Bounds that the kernel tests do not already own (tests/_numerics.py holds the derivations):

* a training BatchNorm's coefficients and running statistics come from the conv's own fp32-chained statistics while
  the reference sums the stored y in fp64: ``finalize_carried`` carries ``assert_conv_stats``'s allowance
  ((rows + 4) * u * sum|term|) through mean, variance, invstd, scale, shift and the running statistics;
* dgamma / dbeta / bcoef come from BN-backward sums taken in a data-gradient epilogue before the 16-bit rounding of dz:
  ``check_bwd_finalize_carried`` carries ``assert_bnb_sums``'s bounds (element bound of dz summed + fp32 chain);
* an element whose fp64 pre-activation lies within 3u * (|scale * y| + |shift|) of zero may take either ReLU branch
  (the fp32 evaluation is one fma or a multiply and an add: at most 2 roundings, margin 1.5); such elements are left out
  of the element comparison, enter the sums' bounds with their whole magnitude, and may be at most 1e-3 of a tensor.

Deliberate departures of the executor from nn.BatchNorm2d / autograd, encoded here instead of tolerated:

* the returned fp32 logits, the loss and the accuracy are formed from the 16-bit ``logits`` buffer plus the fp32 fc bias
  (executor.py ``_loss``: ``xent`` reads ``saved["logits"]``), so the reference starts from the recorded 16-bit logits;
* ``num_batches_tracked`` is kept by the trainer, not the executor: the audit judges running_mean / running_var only
  and requires num_batches_tracked unchanged by the step.
"""
import math
from collections import namedtuple

import torch

import _conv_cases as cc
import _numerics as nm
import _pool_cases as pc
from _numerics import U

Finding = namedtuple("Finding", "path quantity ratio detail")
MASK_CAP = 1e-3


class StepRecord:
    """Named tensors of one step (``t``), a few flags (``meta``), and what the audit has judged so far."""

    def __init__(self, train):
        self.train = train
        self.t = {}
        self.meta = {}

    def put(self, name, tensor):
        assert name not in self.t, name
        self.t[name] = tensor.detach().clone()

    def has(self, name):
        return name in self.t


def block_paths(model):
    """[(module path, block)] in execution order."""
    return [(f"layer{li}.{i}", blk) for li in (1, 2, 3, 4) for i, blk in enumerate(getattr(model, f"layer{li}"))]


def block_convs(blk):
    n = 3 if hasattr(blk, "conv3") else 2
    return [(getattr(blk, f"conv{i}"), getattr(blk, f"bn{i}")) for i in range(1, n + 1)]


# ====================================================================================================== extraction
def _unpack_bits(mask, shape):
    ar = torch.arange(8, device=mask.device, dtype=torch.uint8)
    return ((mask.reshape(-1, 1) >> ar) & 1).bool().reshape(shape)


def _same(a, t):
    return torch.is_tensor(a) and a.data_ptr() == t.data_ptr() and a.numel() == t.numel() and a.dtype == t.dtype


_DGRADS = ("conv_dgrad", "conv_dgrad_bn", "gconv_dgrad")


def _dgrad_of(tape, dy, after):
    """The data-gradient launch that reads ``dy``, first after call ``after`` (a grouped conv on a degenerate image runs
    slice by slice: the last of the consecutive launches holds every slice)."""
    hit = [c for c in tape.calls if c.index > after and c.name in _DGRADS and _same(c.args[0], dy)]
    assert hit, "no data-gradient launch reads this dY"
    c = hit[0]
    for nxt in hit[1:]:
        if nxt.name == "gconv_dgrad" and nxt.index == c.index + 1:
            c = nxt
    return c


def extract_record(ex, saved, tape, model, train):
    """StepRecord of the step that produced ``saved`` (the return value of ``ex._forward``) and ``tape``."""
    r = StepRecord(train)
    N = saved["N"]
    st = ex.stem
    r.put("input.packed", saved["xp"].view(N, saved["Hp"], saved["Wp"], 4))
    P0, Q0, H1, W1 = saved["P0"], saved["Q0"], saved["H1"], saved["W1"]
    r.put("conv1.y", saved["y0"].view(N, P0, Q0, st.cout))
    r.put("bn1.coef", ex.stem_bn.coef)
    r.put("maxpool.out", saved["x0"].view(N, H1, W1, st.cout))
    r.put("maxpool.idx", saved["idx"].view(N, H1, W1, st.cout))
    paths = block_paths(model)
    assert len(paths) == len(ex.blocks)
    for (path, blk), b, s in zip(paths, ex.blocks, saved["blocks"]):
        for ci, (c, bn) in enumerate(zip(b["convs"], b["bns"])):
            h, w, P, Q = s["hw"][ci]
            r.put(f"{path}.conv{ci + 1}.y", s["ys"][ci].view(N, P, Q, c.cout))
            r.put(f"{path}.bn{ci + 1}.coef", bn.coef)
            if ci < len(b["convs"]) - 1:
                fused = s["pre"][ci] is not None
                r.meta[f"{path}.bn{ci + 1}.fused_into_consumer"] = fused
                if not fused:
                    r.put(f"{path}.bn{ci + 1}.a", s["as"][ci].view(N, P, Q, c.cout))
        P, Q = s["hw"][-1][2], s["hw"][-1][3]
        co = b["convs"][-1].cout
        if b["ds_conv"] is not None:
            r.put(f"{path}.downsample.0.y", s["yd"].view(N, P, Q, co))
            r.put(f"{path}.downsample.1.coef", b["ds_bn"].coef)
        r.put(f"{path}.out", s["out"].view(N, P, Q, co))
        if train:
            r.put(f"{path}.omask", _unpack_bits(s["omask"], (N, P, Q, co)))
    r.put("avgpool.feat", saved["feat"].view(N, ex.feat))
    r.put("fc.logits_pad", saved["logits"].view(N, ex.ncls_pad))
    xe = tape.named("xent")[-1]
    r.put("logits", xe.outs[6])
    r.put("xent.row_loss", xe.outs[10][:N])
    r.put("xent.row_correct", xe.outs[11][:N])
    r.put("met", tape.named("metrics")[-1].outs[3])
    for n, b in model.named_buffers():
        r.put(f"buf:{n}", b)
    if not train:
        return r
    # ------------------------------------------------------------------------------------------------ backward
    r.put("fc.dlogits", xe.outs[7].view(N, ex.ncls_pad))
    dfeat = ex._bufs[("dfeat", ex.dtype)]
    c = [c for c in tape.named("conv_fwd") if c.args[2].data_ptr() == dfeat.data_ptr()][-1]
    r.put("avgpool.dfeat", c.outs[2].view(N, ex.feat))
    Hc, Wc, Cc = saved["Hc"], saved["Wc"], saved["Cc"]
    r.put("head.g", tape.named("avgpool_bwd")[-1].outs[1].view(N, Hc, Wc, Cc))
    applies = tape.named("bn_bwd_apply")
    for (path, blk), b, s in reversed(list(zip(paths, ex.blocks, saved["blocks"]))):
        nconv = len(b["convs"])
        ds = b["ds_conv"] is not None
        ylast = s["ys"][-1]
        ap = [c for c in applies if _same(c.args[2], ylast)]
        assert len(ap) == 1, f"{path}: {len(ap)} bn_bwd_apply launches over the last conv's output"
        ap = ap[0]
        _, _, P, Q = s["hw"][-1]
        co = b["convs"][-1].cout
        r.meta[f"{path}.gin_is_dz"] = ap.args[1] is None
        r.put(f"{path}.bn{nconv}.dy", ap.outs[4].view(N, P, Q, co))
        r.put(f"{path}.bn{nconv}.bcoef", b["bns"][-1].bcoef)
        if ds:
            r.put(f"{path}.downsample.1.dy", ap.outs[7].view(N, P, Q, co))
            r.put(f"{path}.downsample.1.bcoef", b["ds_bn"].bcoef)
            dg = _dgrad_of(tape, ap.args[7], ap.index)
            compact = dg.outs[2].numel() == N * P * Q * s["C"]
            r.meta[f"{path}.downsample.0.dx_compact"] = compact and (P, Q) != (s["H"], s["W"])
            r.put(f"{path}.downsample.0.dx", dg.outs[2].view(N, P, Q, s["C"]) if compact and (P, Q) != (s["H"], s["W"])
                  else dg.outs[2].view(N, s["H"], s["W"], s["C"]))
        elif 8 in ap.outs:
            r.put(f"{path}.dz", ap.outs[8].view(N, P, Q, co))
        dy, after = ap.args[4], ap.index
        for ci in range(nconv - 1, -1, -1):
            cv = b["convs"][ci]
            h, w, _, _ = s["hw"][ci]
            dg = _dgrad_of(tape, dy, after)
            if ci > 0:
                r.put(f"{path}.conv{ci + 1}.dx", dg.outs[2].view(N, h, w, cv.cin))
                ia = [c for c in applies if _same(c.args[2], s["ys"][ci - 1]) and c.index > dg.index]
                assert ia, f"{path}: no bn_bwd_apply over conv{ci}'s output"
                ia = ia[0]
                r.put(f"{path}.bn{ci}.dy", ia.outs[4].view(s["ys"][ci - 1].numel() // cv.cin // (h * w), h, w, cv.cin))
                r.put(f"{path}.bn{ci}.bcoef", b["bns"][ci - 1].bcoef)
                dy, after = ia.args[4], ia.index
            else:
                r.put(f"{path}.gout", dg.outs[2].view(N, h, w, cv.cin))
                r.meta[f"{path}.gout_is_dz"] = dg.name == "conv_dgrad_bn" and dg.args[16] in (2, 3)
    r.put("bn1.bcoef", ex.stem_bn.bcoef)
    sa = tape.named("stem_pool_bwd_apply")
    if sa:
        r.put("conv1.dy", sa[-1].outs[5].view(N, P0, Q0, st.cout))
    for n, p in model.named_parameters():
        r.put(f"grad:{n}", p.grad)
    return r


# ====================================================================================================== the walk
def krsc(conv, dtype, weights=None):
    """The conv's weight as the kernels must see it: rounded to ``dtype``, fp64, KRSC; a grouped conv as the dense
    block-diagonal [cout, R, S, cin] weight."""
    w = (conv.weight if weights is None else weights).detach().to(dtype).double()
    G = conv.groups
    if G == 1:
        return w.permute(0, 2, 3, 1).contiguous()
    co, cg, R, S = w.shape
    og = co // G
    dense = torch.zeros(co, R, S, cg * G, dtype=torch.float64, device=w.device)
    for g in range(G):
        dense[g * og:(g + 1) * og, :, :, g * cg:(g + 1) * cg] = w[g * og:(g + 1) * og].permute(0, 2, 3, 1)
    return dense


def grouped_diag(dense, conv):
    """[cout, R, S, cin] dense -> the grouped parameter's logical [cout, cg, R, S]."""
    G = conv.groups
    co, R, S, ci = dense.shape
    if G == 1:
        return dense.permute(0, 3, 1, 2)
    og, cg = co // G, ci // G
    return torch.cat([dense[g * og:(g + 1) * og, :, :, g * cg:(g + 1) * cg] for g in range(G)], 0).permute(0, 3, 1, 2)


def pre_mask(y, coef, C):
    """(fp64 pre-activation > 0, undecided) of relu(y * scale + shift) from the fp32 coefficients."""
    c64 = coef.double()
    t = y.double() * c64[:C]
    pre, mag = t + c64[C:2 * C], t.abs() + c64[C:2 * C].abs()
    return pre > 0, pre.abs() <= 3 * U * mag


def fused_input(y, coef, C, dtype):
    """relu(bn(y)) as a consumer that applies the producer BN itself forms it: one fp32 fma rounded to ``dtype``
    (tests/_conv_cases.py pre_apply_ref, any width)."""
    c64 = coef.double()
    return torch.relu(y.double() * c64[:C] + c64[C:2 * C]).float().to(dtype)


class _Walk:
    def __init__(self, rec, model, dtype, fam):
        self.rec, self.model, self.dtype, self.fam = rec, model, dtype, fam
        self.findings = []
        self.judged = {}
        self.worst = {}

    def t(self, name):
        return self.rec.t[name]

    def judge(self, names, path, quantity, fn):
        """Run one check (``fn`` returns its worst ratio); ``names``: the record entries it judges."""
        try:
            ratio = float(fn() or 0.0)
            detail = ""
        except AssertionError as e:
            ratio, detail = float("inf"), str(e)
            self.findings.append(Finding(path, quantity, ratio, detail))
        for n in ([names] if isinstance(names, str) else names):
            self.judged[n] = max(self.judged.get(n, 0.0), ratio)

    def family(self, kind):
        return f"{self.fam}/{kind}"


def _exact(got, ref, name):
    g, r = got.double().reshape(-1), ref.double().reshape(-1)
    bad = (g != r) | torch.isnan(g)
    n = int(bad.sum())
    if n:
        i = int(bad.nonzero()[0])
        raise AssertionError(f"{name}: {n} of {g.numel()} elements differ; first element {i}: got {g[i].item()!r}, "
                             f"expected {r[i].item()!r}")
    return 0.0


def _masked_compare(got, ref, bound, unsure, name, C, family):
    share = float(unsure.double().mean())
    assert share <= MASK_CAP, f"{name}: {share:.5f} of the pre-activations are too close to zero to call"
    g = torch.where(unsure, ref, got.double())
    return nm.assert_within(g, ref, bound, name, C, family, ref.shape)


def audit(record, model, buffers_before, images, target, dtype, train=True, loss_scale=None, grad_div=None,
          syncbn_world=None, family="step"):
    """Judge every tensor of ``record``; returns the list of Findings (empty: the step is right).  ``buffers_before``:
    {buffer name: value before the step}.  ``syncbn_world``: None without SyncBN, else the world size (identical batches
    on every rank: the statistics' sums and counts are multiplied by it, dgamma / dbeta are the local share)."""
    rec = record
    wk = _Walk(rec, model, dtype, family)
    t, judge, fam = wk.t, wk.judge, wk.family
    dev = t("conv1.y").device
    world = int(syncbn_world) if syncbn_world else 1
    N = images.shape[0]
    f64 = lambda v: v.detach().to(dev).double()

    # ---------------------------------------------------------------------------------------------- helpers
    def bn_forward(path, bn, y, coef_name):
        """Training: coef and running statistics from the recorded y; eval: coef from the buffers."""
        C = bn.num_features
        coef = t(coef_name)
        rm0, rv0 = buffers_before[f"{path}.running_mean"].to(dev), buffers_before[f"{path}.running_var"].to(dev)
        names = [coef_name, f"buf:{path}.running_mean", f"buf:{path}.running_var", f"buf:{path}.num_batches_tracked"]

        def run():
            rm, rv = t(f"buf:{path}.running_mean"), t(f"buf:{path}.running_var")
            # num_batches_tracked is the trainer's (module docstring): the executor must leave it alone
            _exact(t(f"buf:{path}.num_batches_tracked"), buffers_before[f"{path}.num_batches_tracked"].to(dev),
                   f"{path}: num_batches_tracked")
            if not train:
                _exact(rm, rm0, f"{path}: running_mean (eval)")
                _exact(rv, rv0, f"{path}: running_var (eval)")
                eps32 = float(torch.tensor(bn.eps, dtype=torch.float32))
                invstd = 1.0 / torch.sqrt(rv0.double() + eps32)
                scale = f64(bn.weight) * invstd
                shift = f64(bn.bias) - rm0.double() * scale
                fm = fam("eval_coef")
                w = nm.assert_within(coef[3 * C:], invstd, 8 * U * invstd.abs(), f"{path}: eval invstd", C, fm)
                w = max(w, nm.assert_within(coef[:C], scale, 8 * U * scale.abs(), f"{path}: eval scale", C, fm))
                w = max(w, nm.assert_within(coef[C:2 * C], shift, 10 * U * (f64(bn.bias).abs() + (rm0.double() * scale).abs()),
                                            f"{path}: eval shift", C, fm))
                _exact(coef[2 * C:3 * C], rm0, f"{path}: eval mean")
                return w
            y64 = y.double().reshape(-1, C)
            rows = y64.shape[0]
            count = float(rows * world)
            s, ss = y64.sum(0) * world, (y64 * y64).sum(0) * world
            mom = bn.momentum if bn.momentum is not None else 0.1
            ref = nm.bn_finalize_ref(s, ss, count, f64(bn.weight), f64(bn.bias), bn.eps, mom, rm0, rv0)
            allow = (rows + 4) * U * world
            car = nm.finalize_carried(ref, allow * y64.abs().sum(0), allow * (y64 * y64).sum(0), count, f64(bn.weight),
                                      bn.eps, mom)
            return nm.check_finalize_carried(coef, rm, rv, ref, car, C, path, fam("finalize"))
        judge(names, path, "coef / running statistics", run)

    def conv_forward(path, conv, x, y_name):
        w = krsc(conv, dtype)
        n = conv.kernel_size[0] * conv.kernel_size[1] * conv.in_channels // conv.groups

        def run():
            ref, mag = nm.conv_fwd_ref(x, w, conv.stride[0], conv.padding[0])
            return nm.assert_conv(t(y_name), ref, mag, n, dtype, f"{path}: y", fam("conv_fwd"))
        judge(y_name, path, "y", run)

    def bn_backward(path, bn, dz_ref, sum_bound, y, coef, bcoef_name, rows):
        """dgamma, dbeta and bcoef of ``bn`` from the reference dz [rows, C] (``sum_bound``: its element bound, None:
        dz is exact)."""
        C = bn.num_features
        xh = nm.bn_xhat(y, coef, C)
        dz = dz_ref.reshape(-1, C)
        tt = dz * xh
        sb = torch.zeros_like(dz) if sum_bound is None else sum_bound.reshape(-1, C)
        b0 = (sb.sum(0) + (rows + 4) * U * dz.abs().sum(0)) * world
        b1 = ((sb * xh.abs()).sum(0) + (rows + 4) * U * tt.abs().sum(0)) * world
        count = float(rows * world)
        ref = nm.bn_bwd_finalize_ref(dz.sum(0) * world, tt.sum(0) * world, count, coef, f64(bn.weight), 1.0 / world, C)
        names = [bcoef_name, f"grad:{path}.weight", f"grad:{path}.bias"]
        judge(names, path, "dgamma / dbeta / bcoef", lambda: nm.check_bwd_finalize_carried(
            t(bcoef_name), t(f"grad:{path}.weight"), t(f"grad:{path}.bias"), ref, b0, b1, count, 1.0 / world, coef, C,
            path, fam("bwd_finalize")))

    def bwd_apply(path, dz, y, bcoef, dy_name, C):
        def run():
            ref, mag = nm.bn_bwd_apply_ref(dz.double(), y, bcoef, C)
            return nm.assert_rounded(t(dy_name).reshape(-1, C), ref, mag, dtype, 8, f"{path}: dy", C, fam("bwd_apply"))
        judge(dy_name, path, "dy", run)

    def wgrad(path, conv, x, dy):
        R, S = conv.kernel_size
        n = dy.shape[0] * dy.shape[1] * dy.shape[2]

        def run():
            ref, _ = nm.conv_wgrad_ref(x, dy, R, S, conv.stride[0], conv.padding[0])
            # the wgrad tests' bound; unscaled fp16 gradients are subnormal operands, whose sums the MFMA keeps to an
            # ulp of the NOMINAL magnitudes (tests/_numerics.py): the same for normal operands
            mag = nm.conv_wgrad_nominal_mag(x, dy, R, S, conv.stride[0], conv.padding[0], dtype)
            ref, mag = grouped_diag(ref, conv), grouped_diag(mag, conv)
            got = t(f"grad:{path}.weight")
            assert got.shape == ref.shape, f"{path}: gradient shape {tuple(got.shape)}"
            # (channel-last view so the failure's index reads (k, r, s, c))
            return nm.assert_conv(got.permute(0, 2, 3, 1), ref.permute(0, 2, 3, 1).contiguous(),
                                  mag.permute(0, 2, 3, 1).contiguous(), n, torch.float32, f"{path}: weight gradient",
                                  fam("wgrad"))
        judge(f"grad:{path}.weight", path, "weight gradient", run)

    # ---------------------------------------------------------------------------------------------- stem forward
    c1 = model.conv1
    pad = c1.padding[0]
    H, W = images.shape[2], images.shape[3]
    xp = t("input.packed")
    if images.dtype == torch.uint8:
        from pytorch_distributed_template_amd.data.transforms import IMAGENET_MEAN, IMAGENET_STD
        mean = torch.tensor(IMAGENET_MEAN, dtype=torch.float64, device=dev).view(1, 3, 1, 1)
        std = torch.tensor(IMAGENET_STD, dtype=torch.float64, device=dev).view(1, 3, 1, 1)
        xd = images.to(dev).double()
        img_ref, img_mag = (xd / 255.0 - mean) / std, (xd / (255.0 * std)).abs() + (mean / std).abs()
    else:
        img_ref = images.to(dev).float().to(dtype).double()  # a cast: exact
        img_mag = None

    def packed():
        assert xp.shape[1] >= H + 2 * pad and xp.shape[2] >= W + 2 * pad and xp.shape[3] == 4
        exp = torch.zeros(xp.shape, dtype=torch.float64, device=dev)
        exp[:, pad:pad + H, pad:pad + W, :3] = img_ref.permute(0, 2, 3, 1)
        if img_mag is None:
            return _exact(xp, exp, "packed image")
        border = torch.ones(xp.shape, dtype=torch.bool, device=dev)
        border[:, pad:pad + H, pad:pad + W, :3] = False
        _exact(xp[border], exp[border], "packed image: border and fourth channel")
        mg = torch.zeros_like(exp)
        mg[:, pad:pad + H, pad:pad + W, :3] = img_mag.permute(0, 2, 3, 1)
        return nm.assert_rounded(xp, exp, mg, dtype, 8, "packed image", 4, fam("pack_u8"))
    judge("input.packed", "conv1", "packed image", packed)
    x_img = xp[:, pad:pad + H, pad:pad + W, :3].contiguous()
    conv_forward("conv1", c1, x_img, "conv1.y")
    y0, coef0 = t("conv1.y"), t("bn1.coef")
    bn_forward("bn1", model.bn1, y0, "bn1.coef")
    C0 = c1.out_channels

    def pool():
        r = pc.pool_fwd_ref(y0, coef0, 3, 1)
        return pc.assert_pool_fwd(t("maxpool.out"), t("maxpool.idx"), r, dtype, 255, "maxpool", fam("pool"))
    judge(["maxpool.out", "maxpool.idx"], "maxpool", "out / argmax", pool)

    # ---------------------------------------------------------------------------------------------- blocks forward
    x = t("maxpool.out")
    blocks = block_paths(model)
    for path, blk in blocks:
        cur = x
        cbs = block_convs(blk)
        for i, (conv, bn) in enumerate(cbs, 1):
            conv_forward(f"{path}.conv{i}", conv, cur, f"{path}.conv{i}.y")
            y, coef = t(f"{path}.conv{i}.y"), t(f"{path}.bn{i}.coef")
            bn_forward(f"{path}.bn{i}", bn, y, f"{path}.bn{i}.coef")
            C = conv.out_channels
            if i < len(cbs):
                if rec.meta.get(f"{path}.bn{i}.fused_into_consumer"):
                    cur = fused_input(y, coef, C, dtype)
                else:
                    def run(y=y, coef=coef, C=C, name=f"{path}.bn{i}.a"):
                        _, ref, mag = nm.bn_apply_ref(y, coef, None, None, C, 0, True)
                        return nm.assert_rounded(t(name).reshape(-1, C), ref, mag, dtype, 8, name, C, fam("apply"))
                    judge(f"{path}.bn{i}.a", f"{path}.bn{i}", "a", run)
                    cur = t(f"{path}.bn{i}.a")
        nl = len(cbs)
        ylast, clast = t(f"{path}.conv{nl}.y"), t(f"{path}.bn{nl}.coef")
        C = ylast.shape[-1]
        if blk.downsample is not None:
            conv_forward(f"{path}.downsample.0", blk.downsample[0], x, f"{path}.downsample.0.y")
            yd, cd = t(f"{path}.downsample.0.y"), t(f"{path}.downsample.1.coef")
            bn_forward(f"{path}.downsample.1", blk.downsample[1], yd, f"{path}.downsample.1.coef")
            res, rcoef, mode = yd, cd, 2
        else:
            res, rcoef, mode = x, None, 1

        def run(ylast=ylast, clast=clast, res=res, rcoef=rcoef, mode=mode, C=C, name=f"{path}.out"):
            _, ref, mag = nm.bn_apply_ref(ylast, clast, res, rcoef, C, mode, True)
            return nm.assert_rounded(t(name).reshape(-1, C), ref, mag, dtype, 8, name, C, fam("apply"))
        judge(f"{path}.out", path, "out", run)
        x = t(f"{path}.out")
        if train:
            judge(f"{path}.omask", path, "omask", lambda x=x, name=f"{path}.omask": _exact(t(name), x > 0, name))

    # ---------------------------------------------------------------------------------------------- head
    fc = model.fc
    ncls, F_ = fc.out_features, fc.in_features
    HW = x.shape[1] * x.shape[2]

    def feat():
        x64 = x.double().reshape(N, HW, -1)
        ref = x64.mean(1)
        return nm.assert_within(t("avgpool.feat"), ref, nm.half_ulp16(ref, dtype) + (HW + 2) * U * x64.abs().sum(1) / HW,
                                "avgpool feat", F_, fam("head"))
    judge("avgpool.feat", "avgpool", "feat", feat)
    wfc = fc.weight.detach().to(dev).to(dtype).double()  # [ncls, F]
    lp = t("fc.logits_pad")

    def logits_pad():
        f64_ = t("avgpool.feat").double()
        ref, mag = f64_ @ wfc.t(), f64_.abs() @ wfc.abs().t()
        _exact(lp[:, ncls:], torch.zeros_like(lp[:, ncls:]), "fc: padded class columns")  # no bias in this buffer
        return nm.assert_within(lp[:, :ncls], ref, nm.conv_bound(ref, mag, F_, dtype), "fc logits", ncls, fam("head"))
    judge("fc.logits_pad", "fc", "logits (padded, no bias)", logits_pad)
    gs = (float(loss_scale) if loss_scale is not None else 1.0) / float(grad_div or N)
    # the loss, the accuracy and the returned logits start from the 16-bit logits (module docstring); only the first
    # ncls columns take part
    xr = nm.xent_ref(lp, fc.bias.detach().to(dev), target.to(dev), ncls, gs, dtype)

    def xent():
        w = nm.assert_rounded(t("logits"), xr["v"], xr["vmag"], torch.float32, 1, "returned logits", ncls, fam("xent"))
        w = max(w, nm.assert_within(t("xent.row_loss"), xr["loss"], xr["loss_bound"], "row loss", None, fam("xent")))
        _exact(t("xent.row_correct"), xr["correct"], "row correct")
        return w
    judge(["logits", "xent.row_loss", "xent.row_correct"], "fc", "logits / loss / correct", xent)

    def met():
        rl, rc = t("xent.row_loss").double(), t("xent.row_correct").double()
        ref = torch.stack([rl.mean(), rc.mean()])  # unscaled: loss_scale and grad_div touch the gradients only
        return nm.assert_sum(t("met"), ref, torch.stack([rl.abs().mean(), rc.mean()]), math.ceil(N / 256) + 9, "met", 2,
                             fam("xent"))
    judge("met", "fc", "met", met)
    if not train:
        return _finish(wk)

    # ---------------------------------------------------------------------------------------------- head backward
    dl = t("fc.dlogits")

    def dlogits():
        _exact(dl[:, ncls:], torch.zeros_like(dl[:, ncls:]), "dlogits: padded class columns")
        return nm.assert_within(dl[:, :ncls], xr["dlogits"], xr["dlogits_bound"], "dlogits", ncls, fam("xent"))
    judge("fc.dlogits", "fc", "dlogits", dlogits)
    d64 = dl[:, :ncls].double()
    fe = t("avgpool.feat").double()
    judge("grad:fc.bias", "fc", "bias gradient", lambda: nm.assert_sum(
        t("grad:fc.bias"), d64.sum(0), d64.abs().sum(0), N + 31, "fc bias gradient", ncls, fam("head_bwd")))
    # (the same weight-gradient kernels: nominal magnitudes where an fp16 operand is subnormal, tests/_numerics.py)
    judge("grad:fc.weight", "fc", "weight gradient", lambda: nm.assert_within(
        t("grad:fc.weight"), d64.t() @ fe, nm.conv_bound(d64.t() @ fe, nm.nominal16(d64, dtype).t() @ nm.nominal16(fe, dtype),
                                                        N, torch.float32),
        "fc weight gradient", F_, fam("head_bwd"), (ncls, F_)))

    def dfeat():
        ref, mag = d64 @ wfc, d64.abs() @ wfc.abs()
        return nm.assert_within(t("avgpool.dfeat"), ref, nm.conv_bound(ref, mag, ncls, dtype), "dfeat", F_, fam("head_bwd"))
    judge("avgpool.dfeat", "fc", "dfeat", dfeat)

    def ghead():
        ref = (t("avgpool.dfeat").double() / HW).view(N, 1, 1, -1).expand(t("head.g").shape)
        return nm.assert_within(t("head.g"), ref, nm.half_ulp16(ref, dtype) + 2 * U * ref.abs(), "g", F_, fam("head_bwd"))
    judge("head.g", "avgpool", "g", ghead)

    # ---------------------------------------------------------------------------------------------- blocks backward
    g = t("head.g")
    for bi in range(len(blocks) - 1, -1, -1):
        path, blk = blocks[bi]
        cbs = block_convs(blk)
        nl = len(cbs)
        xin = t(f"{blocks[bi - 1][0]}.out") if bi > 0 else t("maxpool.out")
        out = t(f"{path}.out")
        ylast, clast = t(f"{path}.conv{nl}.y"), t(f"{path}.bn{nl}.coef")
        C = ylast.shape[-1]
        rows = ylast.numel() // C
        is_dz = rec.meta[f"{path}.gin_is_dz"]
        dz = g.double() if is_dz else torch.where(out > 0, g.double(), torch.zeros((), dtype=torch.float64, device=dev))
        ds = blk.downsample is not None
        if not is_dz:  # separate reduce over g and the mask: dz is exact (fused: judged with the dgrad that made g)
            bn_backward(f"{path}.bn{nl}", cbs[-1][1], dz, None, ylast, clast, f"{path}.bn{nl}.bcoef", rows)
            if ds:
                bn_backward(f"{path}.downsample.1", blk.downsample[1], dz, None, t(f"{path}.downsample.0.y"),
                            t(f"{path}.downsample.1.coef"), f"{path}.downsample.1.bcoef", rows)
        bwd_apply(f"{path}.bn{nl}", dz, ylast, t(f"{path}.bn{nl}.bcoef"), f"{path}.bn{nl}.dy", C)
        if ds:
            dconv = blk.downsample[0]
            bwd_apply(f"{path}.downsample.1", dz, t(f"{path}.downsample.0.y"), t(f"{path}.downsample.1.bcoef"),
                      f"{path}.downsample.1.dy", C)
            dyd = t(f"{path}.downsample.1.dy")
            wgrad(f"{path}.downsample.0", dconv, xin, dyd)
            compact = rec.meta[f"{path}.downsample.0.dx_compact"]

            def dsdx(dconv=dconv, dyd=dyd, compact=compact, name=f"{path}.downsample.0.dx"):
                ref, mag = nm.conv_dgrad_ref(dyd, krsc(dconv, dtype), xin.shape[1], xin.shape[2], dconv.stride[0],
                                             dconv.padding[0])
                if compact:  # only phase (0, 0) of a 1x1 strided conv's data gradient is nonzero and written
                    s_ = dconv.stride[0]
                    ref, mag = ref[:, ::s_, ::s_].contiguous(), mag[:, ::s_, ::s_].contiguous()
                n = dconv.out_channels * dconv.kernel_size[0] * dconv.kernel_size[1]
                return nm.assert_conv(t(name), ref, mag, n, dtype, name, fam("dgrad"))
            judge(f"{path}.downsample.0.dx", f"{path}.downsample.0", "data gradient", dsdx)
            residual = t(f"{path}.downsample.0.dx")
            if compact:  # the consumer adds it on phase (0, 0) of the downsample stride
                full_res = torch.zeros(xin.shape, dtype=torch.float64, device=dev)
                full_res[:, ::dconv.stride[0], ::dconv.stride[0]] = residual.double()
                residual = full_res
        else:
            if rec.has(f"{path}.dz"):
                judge(f"{path}.dz", path, "dz", lambda dz=dz, name=f"{path}.dz": _exact(t(name), dz, name))
            residual = dz
        dy = t(f"{path}.bn{nl}.dy")
        for i in range(nl, 0, -1):
            conv, bn = cbs[i - 1]
            cpath = f"{path}.conv{i}"
            if i > 1:
                yp, cp = t(f"{path}.conv{i - 1}.y"), t(f"{path}.bn{i - 1}.coef")
                Cp = yp.shape[-1]
                xc = fused_input(yp, cp, Cp, dtype) if rec.meta.get(f"{path}.bn{i - 1}.fused_into_consumer") \
                    else t(f"{path}.bn{i - 1}.a")
            else:
                xc = xin
            wgrad(cpath, conv, xc, dy)
            w = krsc(conv, dtype)
            n = conv.out_channels // conv.groups * conv.kernel_size[0] * conv.kernel_size[1]
            if i > 1:
                ref, mag = nm.conv_dgrad_ref(dy, w, xc.shape[1], xc.shape[2], conv.stride[0], conv.padding[0])
                mask, unsure = pre_mask(yp, cp, Cp)
                full = nm.conv_bound(ref, mag, n, dtype)
                zero = torch.zeros((), dtype=torch.float64, device=dev)
                dzr, bound = torch.where(mask, ref, zero), torch.where(mask, full, zero)
                judge(f"{cpath}.dx", cpath, "data gradient (masked)", lambda dzr=dzr, bound=bound, unsure=unsure, Cp=Cp,
                      name=f"{cpath}.dx": _masked_compare(t(name), dzr, bound, unsure, name, Cp, fam("dgrad")))
                sb = torch.where(unsure, ref.abs() + full, bound)
                bn_backward(f"{path}.bn{i - 1}", cbs[i - 2][1], dzr, sb, yp, cp, f"{path}.bn{i - 1}.bcoef",
                            yp.numel() // Cp)
                bwd_apply(f"{path}.bn{i - 1}", t(f"{cpath}.dx"), yp, t(f"{path}.bn{i - 1}.bcoef"), f"{path}.bn{i - 1}.dy", Cp)
                dy = t(f"{path}.bn{i - 1}.dy")
            else:
                ref, mag = nm.conv_dgrad_ref(dy, w, xin.shape[1], xin.shape[2], conv.stride[0], conv.padding[0],
                                             residual=residual)
                full = nm.conv_bound(ref, mag, n, dtype)
                gname = f"{path}.gout"
                if rec.meta[f"{path}.gout_is_dz"]:
                    # the buffer already holds dz of the previous block: its output's ReLU (exact from the stored out)
                    ppath, pblk = blocks[bi - 1]
                    pcbs = block_convs(pblk)
                    mask = xin > 0
                    zero = torch.zeros((), dtype=torch.float64, device=dev)
                    dzr, bound = torch.where(mask, ref, zero), torch.where(mask, full, zero)
                    judge(gname, cpath, "data gradient (block input, masked)", lambda dzr=dzr, bound=bound: nm.assert_within(
                        t(gname), dzr, bound, gname, dzr.shape[-1], fam("dgrad"), dzr.shape))
                    pn = len(pcbs)
                    py = t(f"{ppath}.conv{pn}.y")
                    prow = py.numel() // py.shape[-1]
                    bn_backward(f"{ppath}.bn{pn}", pcbs[-1][1], dzr, bound, py, t(f"{ppath}.bn{pn}.coef"),
                                f"{ppath}.bn{pn}.bcoef", prow)
                    if pblk.downsample is not None:
                        bn_backward(f"{ppath}.downsample.1", pblk.downsample[1], dzr, bound, t(f"{ppath}.downsample.0.y"),
                                    t(f"{ppath}.downsample.1.coef"), f"{ppath}.downsample.1.bcoef", prow)
                else:
                    judge(gname, cpath, "data gradient (block input)", lambda ref=ref, mag=mag, n=n: nm.assert_conv(
                        t(gname), ref, mag, n, dtype, gname, fam("dgrad")))
        g = t(f"{path}.gout")
        if bi > 0:
            assert rec.meta[f"{blocks[bi - 1][0]}.gin_is_dz"] == rec.meta[f"{path}.gout_is_dz"], \
                f"{path}: the record disagrees with itself about what the gradient buffer holds"

    # ---------------------------------------------------------------------------------------------- stem backward
    idx, x0 = t("maxpool.idx"), t("maxpool.out")
    P0, Q0 = y0.shape[1], y0.shape[2]
    rows0 = N * P0 * Q0
    prow = N * x0.shape[1] * x0.shape[2]

    def stem_bn():
        ref, mag, carry = pc.pooled_link_ref(y0, coef0, g, idx, x0, 3, 1, dtype)
        b = (torch.stack([(prow + 4) * U * mag[:, 0], (prow + 8) * U * mag[:, 1]], 1) + carry) * world
        count = float(rows0 * world)
        fr = nm.bn_bwd_finalize_ref(ref[:, 0] * world, ref[:, 1] * world, count, coef0, f64(model.bn1.weight), 1.0 / world, C0)
        return nm.check_bwd_finalize_carried(t("bn1.bcoef"), t("grad:bn1.weight"), t("grad:bn1.bias"), fr, b[:, 0], b[:, 1],
                                             count, 1.0 / world, coef0, C0, "bn1", fam("bwd_finalize"))
    judge(["bn1.bcoef", "grad:bn1.weight", "grad:bn1.bias"], "bn1", "dgamma / dbeta / bcoef", stem_bn)
    d = dict(y=y0, dp=g, idx=idx, coef=coef0, b=t("bn1.bcoef"))
    r = cc.stem_tail_ref(d, N, P0, Q0, C0)
    # an element the argmax names was positive in the kernel's fp32: where fp64 cannot call its sign, the gradient the
    # argmax routes there stays (the fused weight gradient takes the mask from the argmax bytes alone)
    b64 = d["b"].double()
    dy_ref = torch.where(r["unsure"], b64[:C0] * r["dzraw"] + b64[C0:2 * C0] * y0.double() + b64[2 * C0:], r["dy"])
    share = float(r["unsure"].double().mean())
    if rec.has("conv1.dy"):
        def dy0():
            assert share <= MASK_CAP, f"conv1.dy: {share:.5f} of the pre-activations are too close to zero to call"
            return pc.assert_tail_apply(t("conv1.dy"), r, dtype, "conv1.dy", fam("stem_tail"))[0]
        judge("conv1.dy", "conv1", "dy", dy0)
        wgrad("conv1", c1, x_img, t("conv1.dy"))
    else:
        def stem_w():
            assert share <= MASK_CAP, f"conv1: {share:.5f} of the pre-activations are too close to zero to call"
            ref, _ = nm.conv_wgrad_ref(x_img, dy_ref, 7, 7, 2, 3)
            bound = nm.stem_fused_bound(x_img, dy_ref, r["dymag"], rows0, dtype)
            return nm.assert_within(t("grad:conv1.weight").permute(0, 2, 3, 1), ref, bound, "conv1: weight gradient", 3,
                                    fam("stem_wgrad"), ref.shape)
        judge("grad:conv1.weight", "conv1", "weight gradient (fused dY)", stem_w)
    return _finish(wk)


def _finish(wk):
    """Completeness: every tensor of the record judged (every parameter gradient and running statistic among them)."""
    rec = wk.rec
    missing = sorted(set(rec.t) - set(wk.judged))
    if missing:
        wk.findings.append(Finding("record", "completeness", float("inf"), f"not judged: {missing}"))
    if rec.train:
        want = [f"grad:{n}" for n, _ in wk.model.named_parameters()]
    else:
        want = []
    want += [f"buf:{n}" for n, _ in wk.model.named_buffers()]
    absent = [n for n in want if n not in wk.judged]
    if absent:
        wk.findings.append(Finding("model", "completeness", float("inf"), f"no judgement of: {absent}"))
    wk.rec.judged = dict(wk.judged)
    return wk.findings


def report(findings, limit=8):
    return "\n".join(f"{f.path}: {f.quantity}: {f.detail[:400]}" for f in findings[:limit]) + \
        (f"\n... and {len(findings) - limit} more" if len(findings) > limit else "")
