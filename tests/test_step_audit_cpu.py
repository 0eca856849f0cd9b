"""CPU proofs of the step audit (tests/_step_audit.py) and of the recording proxy (tests/_tape.py).

``emulate_step`` is a plain torch emulation of one ResNetExecutor training step: fp32 arithmetic, rounded to the 16-bit
type exactly where the executor stores a 16-bit tensor, statistics in fp64 sums finalized in fp32.  It fills the same
``StepRecord`` the GPU extraction fills.  The audit must pass on it, keep the undecided-mask share under its cap and
judge every tensor; and every mutation below -- one wiring error in ONE layer, the kind a whole-network norm absorbs --
must give findings that name that layer and quantity, and none elsewhere.  Teacher forcing makes "elsewhere" strict: a
wrong tensor is the recorded INPUT of the next check, so only checks whose reference does not start from the mutated
tensor itself may fire; the exceptions are listed per mutation in ``MUTATIONS``.
"""
import copy

import pytest
import torch
import torch.nn.functional as F

import _conv_cases as cc
import _numerics as nm
import _pool_cases as pc
import _step_audit as sa
from _tape import Tape

DTYPES = [torch.bfloat16, torch.float16]
NCLS, NPAD = 10, 128


def _model(kind, seed=0):
    from pytorch_distributed_template_amd.models.resnet import BasicBlock, Bottleneck, ResNet
    torch.manual_seed(seed)
    m = ResNet(BasicBlock if kind == "basic" else Bottleneck, [1, 1, 1, 1], num_classes=NCLS)
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.weight.data.uniform_(0.5, 1.5)
            mod.bias.data.uniform_(-0.2, 0.2)
            mod.running_mean.uniform_(-0.5, 0.5)
            mod.running_var.uniform_(0.5, 1.5)
    return m


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def emulate_step(model, images, target, dtype, knobs=None, loss_scale=None, grad_div=None, world=None):
    """One emulated training step (module docstring) -> StepRecord; updates the model's running statistics like the
    executor.  ``knobs``: {"mut": mutation name, "at": module path, ...} applies one wiring error at one layer."""
    kn = knobs or {}
    mut, at = kn.get("mut"), kn.get("at")
    hit = lambda name, path: mut == name and at == path
    r = sa.StepRecord(True)
    N, _, H, W = images.shape
    wsz = world or 1
    rnd = lambda v: v.float().to(dtype)
    w16 = lambda conv, path=None, use=None: (kn["prev_weights"][path] if use else conv.weight.detach()).to(dtype).float()
    means = {}

    def conv_f(x, conv):
        return rnd(_nhwc(F.conv2d(_nchw(x.float()), w16(conv), None, conv.stride, conv.padding, 1, conv.groups)))

    def finalize(path, bn, y):
        C = bn.num_features
        y64 = y.double().reshape(-1, C)
        rows = y64.shape[0]
        count = rows * wsz
        if hit("count_plus_image", path):
            count = count + rows // N
        mean = y64.sum(0) * wsz / count
        var = ((y64 * y64).sum(0) * wsz / count - mean * mean).clamp_min(0)
        eps = 0.0 if hit("eps0", path) else bn.eps
        invstd = (1.0 / torch.sqrt(var + float(torch.tensor(eps).float()))).float()
        mean = mean.float()
        means[path] = mean.clone()
        scale = bn.weight.detach() * invstd
        shift = bn.bias.detach() - mean * scale
        mom = 0.01 if hit("momentum_001", path) else bn.momentum
        unb = var if hit("biased_rv", path) else var * count / (count - 1)
        m_upd = kn["prev_means"][path] if hit("rm_prev_mean", path) else mean
        bn.running_mean.copy_((1 - mom) * bn.running_mean + mom * m_upd)
        bn.running_var.copy_((1 - mom) * bn.running_var + mom * unb.float())
        coef = torch.cat([scale, shift, mean, invstd]).contiguous()
        r.put(f"{path}.coef", coef)
        return coef

    # ------------------------------------------------------------------------------------------------ forward
    c1 = model.conv1
    pad = c1.padding[0]
    xp = torch.zeros(N, H + 2 * pad + 2, W + 2 * pad + 2, 4, dtype=dtype)
    if images.dtype == torch.uint8:
        from pytorch_distributed_template_amd.data.transforms import IMAGENET_MEAN, IMAGENET_STD
        std = torch.tensor(IMAGENET_STD)
        mean_ = torch.tensor(IMAGENET_MEAN)
        if mut == "u8_shift_channel":
            mean_ = mean_.roll(1)
        sc, sh = (1.0 / (255.0 * std)).view(1, 3, 1, 1), (-mean_ / std).view(1, 3, 1, 1)
        img = rnd(images.float() * sc + sh)
    else:
        img = rnd(images)
    xp[:, pad:pad + H, pad:pad + W, :3] = _nhwc(img)
    r.put("input.packed", xp)
    x_img = _nhwc(img)
    y0 = conv_f(x_img, c1)
    r.put("conv1.y", y0)
    coef0 = finalize("bn1", model.bn1, y0)
    x0, idx = pc.pool_fwd_emul(y0, coef0, dtype, 3, 1, 255)
    r.put("maxpool.out", x0)
    r.put("maxpool.idx", idx)
    x = x0
    blocks = sa.block_paths(model)
    fwd = []
    for path, blk in blocks:
        cbs = sa.block_convs(blk)
        cur, ys, coefs, acts = x, [], [], [x]
        for i, (conv, bn) in enumerate(cbs, 1):
            y = conv_f(cur, conv)
            r.put(f"{path}.conv{i}.y", y)
            coef = finalize(f"{path}.bn{i}", bn, y)
            ys.append(y)
            coefs.append(coef)
            if i < len(cbs):
                C = conv.out_channels
                r.meta[f"{path}.bn{i}.fused_into_consumer"] = False
                cur = rnd(nm.bn_apply_emul(y, coef, None, None, C, 0, True)).view(y.shape)
                r.put(f"{path}.bn{i}.a", cur)
                acts.append(cur)
        C = ys[-1].shape[-1]
        yd = cd = None
        if blk.downsample is not None:
            yd = conv_f(x, blk.downsample[0])
            r.put(f"{path}.downsample.0.y", yd)
            cd = finalize(f"{path}.downsample.1", blk.downsample[1], yd)
            val = nm.bn_apply_emul(ys[-1], coefs[-1], yd, cd, C, 2, True)
        else:
            res = ys[0] if hit("residual_neighbour", path) else x
            val = nm.bn_apply_emul(ys[-1], coefs[-1], res, None, C, 1, True)
        out = rnd(val).view(ys[-1].shape)
        r.put(f"{path}.out", out)
        om = out > 0
        if hit("omask_pre_residual", path):
            om = nm.bn_apply_emul(ys[-1], coefs[-1], None, None, C, 0, True).view(out.shape) > 0
        r.put(f"{path}.omask", om)
        fwd.append(dict(x=x, ys=ys, coefs=coefs, acts=acts, yd=yd, cd=cd, out=out, om=om))
        x = out
    fc = model.fc
    HW = x.shape[1] * x.shape[2]
    feat = rnd(x.float().reshape(N, HW, -1).sum(1) * (1.0 / HW))
    r.put("avgpool.feat", feat)
    wfc = fc.weight.detach().to(dtype).float()
    lp = torch.zeros(N, NPAD, dtype=dtype)
    lp[:, :NCLS] = rnd(feat.float() @ wfc.t())
    r.put("fc.logits_pad", lp)
    v = lp[:, :NCLS].float() + fc.bias.detach()
    r.put("logits", v)
    vl = torch.cat([v, lp[:, NCLS:NCLS + 1].float()], 1) if mut == "pad_column_lse" else v
    lse = torch.logsumexp(vl, 1)
    rl = lse - v.gather(1, target.view(-1, 1)).squeeze(1)
    r.put("xent.row_loss", rl)
    rc = (v.argmax(1) == target).float()
    r.put("xent.row_correct", rc)
    r.put("met", torch.stack([rl.mean(), rc.mean()]))
    gd = float(grad_div or N)
    gs = (float(loss_scale) if loss_scale is not None else 1.0) / gd
    dl = torch.zeros(N, NPAD, dtype=dtype)
    dl[:, :NCLS] = rnd((torch.exp(v - lse.view(-1, 1)) - F.one_hot(target, NCLS)) * gs)
    r.put("fc.dlogits", dl)
    # ------------------------------------------------------------------------------------------------ backward
    grads = {}
    d32 = dl[:, :NCLS].float()
    grads["fc.bias"] = d32.sum(0) * (gd / N if mut == "fcb_no_div" else 1.0)
    grads["fc.weight"] = d32.t() @ feat.float()
    dfeat = rnd(d32 @ wfc)
    r.put("avgpool.dfeat", dfeat)
    g = rnd(dfeat.float() / HW).view(N, 1, 1, -1).expand(x.shape).contiguous()
    r.put("head.g", g)

    def bn_bwd(path, bn, dz32, y, coef, rows):
        """sums of the fp32 dz (before its 16-bit rounding) -> dgamma, dbeta, bcoef"""
        C = bn.num_features
        mean, invstd = coef[2 * C:3 * C], coef[3 * C:]
        xh = ((y.float().reshape(-1, C) - mean) * invstd).double()
        d = dz32.double().reshape(-1, C)
        sdz, sdzx = d.sum(0) * wsz, (d * xh).sum(0) * wsz
        count = rows * wsz
        A = bn.weight.detach() * invstd
        mdz, mdzx = (sdz / count).float(), (sdzx / count).float()
        bc = torch.cat([A, -A * invstd * mdzx, -A * mdz + A * invstd * mdzx * mean]).contiguous()
        gsc = 1.0 if hit("dgamma_world", path) else 1.0 / wsz
        grads[f"{path}.weight"] = (sdzx * gsc).float()
        grads[f"{path}.bias"] = (sdz / wsz).float()
        return bc

    def bwd_apply(dz, y, bc, C):
        return rnd(bc[:C] * dz.float().reshape(-1, C) + bc[C:2 * C] * y.float().reshape(-1, C) + bc[2 * C:]).view(y.shape)

    def dgrad(dy, conv, path, shape):
        w = w16(conv, path, hit("stale_dgrad_weights", path))
        return _nhwc(torch.nn.grad.conv2d_input((shape[0], shape[3], shape[1], shape[2]), w, _nchw(dy.float()),
                                                conv.stride, conv.padding, 1, conv.groups))

    def wgrad(path, conv, x_, dy):
        grads[f"{path}.weight"] = torch.nn.grad.conv2d_weight(_nchw(x_.float()), conv.weight.shape, _nchw(dy.float()),
                                                              conv.stride, conv.padding, 1, conv.groups)

    pending = None  # bcoefs of the block whose output-BN sums came out of the next block's first dgrad
    for bi in range(len(blocks) - 1, -1, -1):
        path, blk = blocks[bi]
        f = fwd[bi]
        cbs = sa.block_convs(blk)
        nl = len(cbs)
        ylast, clast = f["ys"][-1], f["coefs"][-1]
        C = ylast.shape[-1]
        rows = ylast.numel() // C
        fused_in = bi < len(blocks) - 1  # g already holds dz (the route of the default executor)
        r.meta[f"{path}.gin_is_dz"] = fused_in
        ds = blk.downsample is not None
        if fused_in:
            dz = g
            bcl, bcd = pending
        else:
            dz = torch.where(f["om"], g, torch.zeros((), dtype=dtype))
            bcl = bn_bwd(f"{path}.bn{nl}", cbs[-1][1], dz.float(), ylast, clast, rows)
            bcd = bn_bwd(f"{path}.downsample.1", blk.downsample[1], dz.float(), f["yd"], f["cd"], rows) if ds else None
        r.put(f"{path}.bn{nl}.bcoef", bcl)
        if ds:
            r.put(f"{path}.downsample.1.bcoef", bcd)
            if hit("bcoef_swapped", path):
                bcl, bcd = bcd, bcl
        dy = bwd_apply(dz, ylast, bcl, C)
        r.put(f"{path}.bn{nl}.dy", dy)
        if ds:
            dconv = blk.downsample[0]
            dyd = bwd_apply(dz, f["yd"], bcd, C)
            r.put(f"{path}.downsample.1.dy", dyd)
            wgrad(f"{path}.downsample.0", dconv, f["x"], dyd)
            full = dgrad(dyd, dconv, f"{path}.downsample.0", f["x"].shape)
            c0 = cbs[0][0]  # compact only where phase 0 of a 3x3/2 first conv adds it (executor.py compact_ds)
            compact = dconv.stride[0] == 2 and c0.stride[0] == 2 and c0.kernel_size[0] == 3
            r.meta[f"{path}.downsample.0.dx_compact"] = compact
            dsdx = rnd(full[:, ::2, ::2] if compact else full).contiguous()
            r.put(f"{path}.downsample.0.dx", dsdx)
            res32 = torch.zeros(f["x"].shape)
            if compact:
                res32[:, ::2, ::2] = dsdx.float()
            else:
                res32 = dsdx.float()
        else:
            if not fused_in:
                r.put(f"{path}.dz", dz)
            res32 = dz.float()
        for i in range(nl, 0, -1):
            conv = cbs[i - 1][0]
            cpath = f"{path}.conv{i}"
            xc = f["acts"][i - 1]
            wgrad(cpath, conv, xc, dy)
            d32_ = dgrad(dy, conv, cpath, xc.shape)
            if i > 1:
                yp, cp = f["ys"][i - 2], f["coefs"][i - 2]
                Cp = yp.shape[-1]
                pre = yp.float() * cp[:Cp] + cp[Cp:2 * Cp]
                dz32 = torch.where(pre > 0, d32_, torch.zeros(()))
                r.put(f"{cpath}.dx", rnd(dz32))
                bc = bn_bwd(f"{path}.bn{i - 1}", cbs[i - 2][1], dz32, yp, cp, yp.numel() // Cp)
                r.put(f"{path}.bn{i - 1}.bcoef", bc)
                dy = bwd_apply(rnd(dz32), yp, bc, Cp)
                r.put(f"{path}.bn{i - 1}.dy", dy)
            else:
                tot = d32_ + res32
                if bi > 0:
                    pf = fwd[bi - 1]
                    ppath, pblk = blocks[bi - 1]
                    pcbs = sa.block_convs(pblk)
                    tot = torch.where(pf["om"], tot, torch.zeros(()))
                    prow = tot.numel() // tot.shape[-1]
                    pending = (bn_bwd(f"{ppath}.bn{len(pcbs)}", pcbs[-1][1], tot, pf["ys"][-1], pf["coefs"][-1], prow),
                               bn_bwd(f"{ppath}.downsample.1", pblk.downsample[1], tot, pf["yd"], pf["cd"], prow)
                               if pblk.downsample is not None else None)
                r.meta[f"{path}.gout_is_dz"] = bi > 0
                g = rnd(tot)
                r.put(f"{path}.gout", g)
    # stem: sums over the pooled elements with the BN input recovered from the pooled output (the executor's
    # stem_pool_bwd_reduce_out), dY formed in fp32 and rounded to 16 bits for the weight gradient
    C0 = c1.out_channels
    sc, sh, mean0, inv0 = coef0[:C0], coef0[C0:2 * C0], coef0[2 * C0:3 * C0], coef0[3 * C0:]
    live = x0 > 0
    dzp = torch.where(live, g.float(), torch.zeros(()))
    xh = ((x0.float() - sh) / sc - mean0) * inv0
    P0, Q0 = y0.shape[1], y0.shape[2]
    sdz, sdzx = dzp.double().reshape(-1, C0).sum(0) * wsz, (dzp * xh).double().reshape(-1, C0).sum(0) * wsz
    count = N * P0 * Q0 * wsz
    A = model.bn1.weight.detach() * inv0
    mdz, mdzx = (sdz / count).float(), (sdzx / count).float()
    bc0 = torch.cat([A, -A * inv0 * mdzx, -A * mdz + A * inv0 * mdzx * mean0]).contiguous()
    grads["bn1.weight"], grads["bn1.bias"] = (sdzx / wsz).float(), (sdz / wsz).float()
    r.put("bn1.bcoef", bc0)
    tail = cc.stem_tail_ref(dict(y=y0, dp=g, idx=idx, coef=coef0, b=bc0), N, P0, Q0, C0)
    dy0 = rnd(bc0[:C0] * tail["dzraw"].float() + bc0[C0:2 * C0] * y0.float() + bc0[2 * C0:])
    wgrad("conv1", c1, x_img, dy0)
    if mut == "stem_tap":
        gw = grads["conv1.weight"]
        gw[5, 1, 3, 4] += gw[5, 1, 3, 3]
        gw[5, 1, 3, 3] = 0.0
    if mut == "swap_grads":
        a, b = kn["swap"]
        grads[a], grads[b] = grads[b], grads[a]
    for n, _ in model.named_parameters():
        r.put(f"grad:{n}", grads[n])
    for n, b in model.named_buffers():
        r.put(f"buf:{n}", b)
    r.means = means
    return r


def _batch(N, HW, seed, u8=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 256, (N, 3, HW, HW), generator=g, dtype=torch.uint8) if u8 else torch.randn(N, 3, HW, HW, generator=g)
    return x, torch.randint(0, NCLS, (N,), generator=g)


def _run(kind, dtype, knobs=None, u8=False, loss_scale=None, grad_div=None, world=None, seed=3):
    model = _model(kind)
    x, t = _batch(2, 32, seed, u8)
    kn = dict(knobs or {})
    with torch.no_grad():
        if kn.get("mut") in ("rm_prev_mean", "stale_dgrad_weights"):
            # "the previous step": another batch's means, and the weights before a parameter update of 1 %
            prev = emulate_step(copy.deepcopy(model), *_batch(2, 32, seed + 1), dtype)
            kn["prev_means"] = prev.means
            g = torch.Generator().manual_seed(9)
            kn["prev_weights"] = {n[:-7]: p.detach() * (1 + 0.01 * torch.randn(p.shape, generator=g))
                                  for n, p in model.named_parameters() if n.endswith(".weight") and p.dim() == 4}
        before = {n: b.clone() for n, b in model.named_buffers()}
        rec = emulate_step(model, x, t, dtype, kn, loss_scale, grad_div, world)
        found = sa.audit(rec, model, before, x, t, dtype, True, loss_scale, grad_div, world, family="step_cpu")
    return rec, found


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["basic", "bottleneck"])
def test_emulated_step_passes_the_audit_and_is_judged_completely(kind, dtype):
    rec, found = _run(kind, dtype)
    assert not found, sa.report(found)
    model = _model(kind)
    for n, _ in model.named_parameters():
        assert f"grad:{n}" in rec.judged, n
    for n, _ in model.named_buffers():
        assert f"buf:{n}" in rec.judged, n
    assert set(rec.t) <= set(rec.judged)
    assert max(rec.judged.values()) <= 1.0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["basic", "bottleneck"])
def test_undecided_masks_stay_under_the_cap_on_the_reference_alone(kind, dtype):
    """The share of elements whose ReLU branch fp32 may call either way, from the record's y and coef alone, for every
    inner BatchNorm and the stem: the seeds the tests use keep it under MASK_CAP."""
    rec, _ = _run(kind, dtype)
    n = 0
    for name, y in rec.t.items():
        if name.endswith(".y") and "downsample" not in name:
            coef = rec.t[("bn1" if name == "conv1.y" else name[:-2].replace("conv", "bn")) + ".coef"]
            _, unsure = sa.pre_mask(y, coef, y.shape[-1])
            assert float(unsure.double().mean()) <= sa.MASK_CAP, name
            n += 1
    assert n >= 9


def test_uint8_loss_scale_and_world_pass():
    for kw in (dict(u8=True), dict(loss_scale=1024.0, grad_div=4.0), dict(world=2), dict(world=1)):
        _, found = _run("basic", torch.float16, **kw)
        assert not found, (kw, sa.report(found))


# mutation -> (net, knobs, extra _run arguments, {path: words one of which the quantity must contain}).  The allowed
# set is exactly what teacher forcing implies:
#  * a wrong coef (count, eps) is judged at its BatchNorm only: the consumers are judged FROM the recorded coef;
#  * residual / mask errors show at the block's out / omask; a wrong omask also moves the recorded dz, which the audit
#    recomputes from the recorded out: the block's dy, dgamma / dbeta / bcoef and (identity block) dz follow;
#  * swapped bcoef: both dy of that block; stale backward-data weights: that conv's data gradient and the BatchNorm
#    finalized from its fused sums;
#  * a pad column in the log-sum-exp moves the row loss and the softmax made from the same sum, i.e. dlogits (met is
#    judged from the recorded rows and stays quiet); an fc bias gradient, a stem tap, the uint8 shift: that quantity
#    alone.
MUTATIONS = {
    "count_plus_image": ("basic", dict(at="layer4.0.bn2"), {}, {"layer4.0.bn2": ["coef"]}),
    "eps0": ("bottleneck", dict(at="layer3.0.bn2"), {}, {"layer3.0.bn2": ["coef"]}),
    "biased_rv": ("basic", dict(at="layer4.0.bn1"), {}, {"layer4.0.bn1": ["coef"]}),
    "momentum_001": ("basic", dict(at="layer2.0.downsample.1"), {}, {"layer2.0.downsample.1": ["coef"]}),
    "rm_prev_mean": ("bottleneck", dict(at="layer1.0.bn3"), {}, {"layer1.0.bn3": ["coef"]}),
    "residual_neighbour": ("basic", dict(at="layer1.0"), {}, {"layer1.0": ["out"]}),
    "omask_pre_residual": ("basic", dict(at="layer1.0"), {}, {"layer1.0": ["omask"], "layer2.0.conv1": ["data gradient"],
                                                              "layer1.0.bn2": ["dgamma"]}),
    "bcoef_swapped": ("basic", dict(at="layer3.0"), {}, {"layer3.0.bn2": ["dy"], "layer3.0.downsample.1": ["dy"]}),
    "stale_dgrad_weights": ("bottleneck", dict(at="layer2.0.conv3"), {}, {"layer2.0.conv3": ["data gradient"],
                                                                          "layer2.0.bn2": ["dgamma"]}),
    "swap_grads": ("basic", dict(swap=("layer1.0.conv1.weight", "layer1.0.conv2.weight")), {},
                   {"layer1.0.conv1": ["weight gradient"], "layer1.0.conv2": ["weight gradient"]}),
    "dgamma_world": ("basic", dict(at="layer2.0.bn1"), dict(world=2), {"layer2.0.bn1": ["dgamma"]}),
    "fcb_no_div": ("basic", {}, dict(loss_scale=1024.0, grad_div=4.0), {"fc": ["bias gradient"]}),
    "pad_column_lse": ("basic", {}, {}, {"fc": ["loss", "dlogits"]}),
    "stem_tap": ("basic", {}, {}, {"conv1": ["weight gradient"]}),
    "u8_shift_channel": ("basic", {}, dict(u8=True), {"conv1": ["packed image"]}),
}
# (residual_neighbour stands for "the residual of a neighbouring tensor of equal shape": with one block per stage the
# identity block has no previous block, so the block's own conv1 output plays the previous block's input.)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mut", sorted(MUTATIONS))
def test_each_wiring_mutation_is_found_at_its_layer(mut, dtype):
    kind, knobs, kw, allowed = MUTATIONS[mut]
    if dtype == torch.bfloat16 and "loss_scale" in kw:
        kw = dict(kw, loss_scale=None)
    _, found = _run(kind, dtype, dict(knobs, mut=mut), **kw)
    assert found, f"{mut}: the audit found nothing"
    first = next(iter(allowed))
    assert any(f.path == first and any(w in f.quantity for w in allowed[first]) for f in found), sa.report(found)
    stray = [f for f in found if not (f.path in allowed and any(w in f.quantity for w in allowed[f.path]))]
    assert not stray, f"{mut}: findings outside the mutated layer:\n" + sa.report(stray)


# ------------------------------------------------------------------------------------------------------ Tape
class _FakeC:
    def __init__(self):
        self.log = []

    def stat_slots(self):
        return 64

    def conv_wgrad_plan(self, *a):
        return (1, 2, 3)

    def conv1x1_c64_supported(self, a, b):
        return True

    def bn_apply(self, y, coef, res, rcoef, out, C, mode, relu, mask):
        out.copy_(y * 2)

    def gconv_dgrad(self, dy, wt, dx, *a, bn_slots=None):
        dx.copy_(dy + 1)
        if bn_slots is not None:
            bn_slots.fill_(7.0)

    def brand_new_kernel(self, x):
        x.zero_()


def test_tape_records_outputs_after_the_call_and_refuses_unknown_launchers():
    tape = Tape(_FakeC())
    assert tape.stat_slots() == 64 and tape.conv_wgrad_plan(1) == (1, 2, 3) and tape.conv1x1_c64_supported(64, 256)
    assert not tape.calls  # queries pass through unrecorded
    y, out = torch.arange(4.0), torch.full((4,), -1.0)
    tape.bn_apply(y, None, None, None, out, 4, 0, True, None)
    c = tape.calls[0]
    assert c.name == "bn_apply" and set(c.outs) == {4} and torch.equal(c.outs[4], y * 2)  # cloned AFTER the call
    out.fill_(5.0)
    assert torch.equal(c.outs[4], y * 2)  # a clone, not a view of the live buffer
    assert torch.equal(tape.value_at(1, out), y * 2) and tape.value_at(0, out) is out
    slots, dx = torch.zeros(3), torch.zeros(4)
    tape.gconv_dgrad(y, None, dx, 1, 2, bn_slots=slots)
    assert set(tape.calls[1].outs) == {2, "bn_slots"} and float(tape.calls[1].outs["bn_slots"][0]) == 7.0
    with pytest.raises(KeyError, match="brand_new_kernel"):
        tape.brand_new_kernel(y)
    assert not hasattr(tape, "no_such_launcher")  # hasattr() of the executor keeps working


def test_nominal_magnitudes_change_nothing_for_normal_operands_and_keep_rejecting_errors():
    """conv_wgrad_nominal_mag (tests/_numerics.py): equal to the plain magnitude where every fp16 operand is a normal
    number and for bf16; with subnormal dY (unscaled fp16 gradients) a gradient element moved to the neighbouring tap,
    one dropped pixel and a one-part-in-1000 error still fail the weight-gradient bound."""
    g = torch.Generator().manual_seed(5)
    x = (torch.rand(3, 4, 4, 16, generator=g) + 0.5).to(torch.float16)
    dy = ((torch.rand(3, 4, 4, 8, generator=g) + 0.5) * 2.0 ** -3).to(torch.float16)
    ref, mag = nm.conv_wgrad_ref(x, dy, 1, 1, 1, 0)
    assert torch.equal(nm.conv_wgrad_nominal_mag(x, dy, 1, 1, 1, 0, torch.float16), mag)
    xb = torch.randn(3, 4, 4, 16, generator=g).to(torch.bfloat16)
    db = (torch.randn(3, 4, 4, 8, generator=g) * 2.0 ** -20).to(torch.bfloat16)
    assert torch.equal(nm.conv_wgrad_nominal_mag(xb, db, 3, 3, 1, 1, torch.bfloat16), nm.conv_wgrad_ref(xb, db, 3, 3, 1, 1)[1])
    x = torch.relu(torch.randn(3, 4, 4, 16, generator=g)).to(torch.float16)
    dy = (torch.randn(3, 4, 4, 8, generator=g) * 2.0 ** -20).to(torch.float16)
    assert float((dy.float().abs() < nm.FP16_MIN_NORMAL).double().mean()) == 1.0
    ref, mag = nm.conv_wgrad_ref(x, dy, 3, 3, 1, 1)
    magn = nm.conv_wgrad_nominal_mag(x, dy, 3, 3, 1, 1, torch.float16)
    assert bool((magn >= mag).all())
    n = 3 * 4 * 4
    good = torch.nn.grad.conv2d_weight(_nchw(x.float()), (8, 16, 3, 3), _nchw(dy.float()), 1, 1).permute(0, 2, 3, 1)
    nm.assert_conv(good, ref, magn, n, torch.float32, "fp32 evaluation", None)
    moved = good.clone()
    moved[2, 1, 1], moved[2, 1, 2] = good[2, 1, 2], good[2, 1, 1]
    drop = torch.nn.grad.conv2d_weight(_nchw(x.float())[:2], (8, 16, 3, 3), _nchw(dy.float())[:2], 1, 1).permute(0, 2, 3, 1)
    for name, bad in (("moved tap", moved), ("dropped image", drop), ("0.1 % error", good * 1.001)):
        with pytest.raises(AssertionError):
            nm.assert_conv(bad, ref, magn, n, torch.float32, name, None)
