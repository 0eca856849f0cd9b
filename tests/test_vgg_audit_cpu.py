"""CPU proofs of the VGG / AlexNet step audit (tests/_vgg_audit.py).

``emulate_step`` is a plain torch emulation of one VGGExecutor step (training or eval): fp32 arithmetic, rounded to the
16-bit type exactly where the executor stores a 16-bit tensor, statistics and backward sums in fp64 finalized in fp32,
dropout from ``vgg_hash_torch``, launches split over image chunks where ``chunked`` says so.  It fills the same
``StepRecord`` the GPU extraction fills.  The audit must pass on it for VGG-bias, VGG-BN and AlexNet in both dtypes, keep
the undecided share under ``MASK_CAP`` and judge every tensor; and every mutation of ``MUTATIONS`` -- one wiring error in
ONE layer -- must give findings that name that layer and quantity, and none elsewhere (teacher forcing: a wrong tensor is
the recorded INPUT of the next check, so only checks whose reference does not start from the mutated tensor may fire;
the exceptions are listed per mutation).
"""
import pytest
import torch
import torch.nn.functional as F

import _conv_cases as cc
import _numerics as nm
import _pool_cases as pc
import _step_audit as sa
import _vgg_audit as va

DTYPES = [torch.bfloat16, torch.float16]
NPAD = 128
CHUNKS = [(0, 2), (2, 3)]


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def emulate_step(model, images, target, dtype, train=True, knobs=None, loss_scale=None, grad_div=None, world=None,
                 chunked=(), seed=1234):
    """One emulated step (module docstring) -> StepRecord; updates the model's running statistics like the executor.
    ``chunked``: indices (into the feature layers) of the convs whose launches run over CHUNKS.  ``knobs``:
    {"mut": mutation name, "at": module path} applies one wiring error at one layer."""
    kn = knobs or {}
    mut, at = kn.get("mut"), kn.get("at")
    hit = lambda name, path: mut == name and at == path
    r = sa.StepRecord(train)
    N, _, H, W = images.shape
    wsz = world or 1
    rnd = lambda v: v.float().to(dtype)
    layers = va.feature_layers(model)
    w16 = lambda m: m.weight.detach().to(dtype).float()
    chunks_of = lambda li: CHUNKS if li in chunked else [(0, N)]

    # ------------------------------------------------------------------------------------------------ forward
    c0 = layers[0].conv
    pad = c0.padding[0]
    xp = torch.zeros(N, H + 2 * pad + 3, W + 2 * pad + 5, 4, dtype=dtype)
    if images.dtype == torch.uint8:
        from pytorch_distributed_template_amd.data.transforms import IMAGENET_MEAN, IMAGENET_STD
        std, mean_ = torch.tensor(IMAGENET_STD), torch.tensor(IMAGENET_MEAN)
        img = rnd(images.float() * (1.0 / (255.0 * std)).view(1, 3, 1, 1) + (-mean_ / std).view(1, 3, 1, 1))
    else:
        img = rnd(images)
    xp[:, pad:pad + H, pad:pad + W, :3] = _nhwc(img)
    r.put("input.packed", xp)
    x = _nhwc(img)
    fwd = []
    for li, L in enumerate(layers):
        P, conv, bn = L.path, L.conv, L.bn
        C = conv.out_channels
        y = rnd(_nhwc(F.conv2d(_nchw(x.float()), w16(conv), None, conv.stride, conv.padding)))
        r.put(f"{P}.y", y)
        r.meta[f"{P}.chunks"] = chunks_of(li)
        bias = conv.bias.detach()
        one, nil = torch.ones(C), torch.zeros(C)
        if bn is None:
            coef = torch.cat([one, bias, nil, one])
        elif train:
            st = []
            for k, (a, b) in enumerate(chunks_of(li)):
                y64 = y[a:b].double().reshape(-1, C)
                st.append(torch.stack([y64.sum(0), (y64 * y64).sum(0)], 1))
                r.put(f"{P}.stats.{k}", st[-1])
            tot = st[0] if hit("stats_chunk2_dropped", P) else sum(st)
            rows = y.numel() // C
            count = rows * wsz
            if hit("count_plus_image", P):
                count += rows // N
            mean = tot[:, 0] * wsz / count
            var = (tot[:, 1] * wsz / count - mean * mean).clamp_min(0)
            invstd = (1.0 / torch.sqrt(var + float(torch.tensor(bn.eps).float()))).float()
            mean = mean.float()
            scale = bn.weight.detach() * invstd
            coef = torch.cat([scale, bn.bias.detach() - mean * scale, mean, invstd])
            mom = bn.momentum
            bn.running_mean.copy_((1 - mom) * bn.running_mean + mom * mean)
            bn.running_var.copy_((1 - mom) * bn.running_var + mom * (var * count / (count - 1)).float())
            if not hit("rm_no_bias", P):
                bn.running_mean.add_(bias, alpha=mom)
        else:
            invstd = 1.0 / torch.sqrt(bn.running_var + float(torch.tensor(bn.eps).float()))
            scale = bn.weight.detach() * invstd
            shift = bn.bias.detach() - bn.running_mean * scale
            if not hit("eval_no_bias", P):
                shift = shift + bias * scale
            coef = torch.cat([scale, shift, bn.running_mean.clone(), invstd])
        coef = coef.contiguous()
        r.put(f"{P}.coef", coef)
        idx = None
        if L.pool:
            act, idx = pc.pool_fwd_emul(y, coef, dtype, L.pool, 0, 255 if L.pool == 3 else None)
            if train or L.pool == 3:
                r.put(f"{P}.idx", idx)
        else:
            act = rnd(nm.bn_apply_emul(y, coef, None, None, C, 0, True)).view(y.shape)
        r.put(f"{P}.act", act)
        fwd.append(dict(x=x, y=y, coef=coef, act=act, idx=idx))
        x = act
    drop0, hidden, (i3, lin3) = va.classifier_plan(model)
    p_model = float([m for m in model.classifier if isinstance(m, torch.nn.Dropout)][0].p)
    dropout = {}

    def fc_act(z, b, p, sd, name):
        dropout[name] = (p, sd)
        thr, scale = pc.dropout_consts(p)
        v = torch.relu(z.float() + b) * scale
        if p > 0:
            v = torch.where((pc.vgg_hash_torch(sd, z.numel(), 0, "cpu") >= thr).view(z.shape), v, torch.zeros(()))
        return v.to(dtype)

    feat = (x if mut == "flatten_nhwc" else x.permute(0, 3, 1, 2)).reshape(N, -1).contiguous()
    r.put("classifier.featc", feat)
    a_in = feat
    pt = p_model if train else 0.0
    if drop0 is not None:
        a_in = fc_act(feat, torch.zeros(feat.shape[1]), pt, seed + 7, f"classifier.{drop0}")
        r.put(f"classifier.{drop0}.x", a_in)
    x0 = a_in
    hs, ps, xins = [], [], []
    for i, (j, lin, dmod) in enumerate(hidden):
        Pj = f"classifier.{j}"
        xins.append(a_in)
        z = rnd(a_in.float() @ w16(lin).t())
        r.put(f"{Pj}.z", z)
        p = pt if (dmod is not None or hit("h2_dropout", Pj)) else 0.0
        sd = seed + (0 if hit("same_seed", Pj) else i)
        a_in = fc_act(z, lin.bias.detach(), p, sd, Pj)
        r.put(f"{Pj}.h", a_in)
        hs.append(a_in)
        ps.append(p)
    r.meta["dropout"] = dropout
    ncls = lin3.out_features
    w3 = w16(lin3)
    lp = torch.zeros(N, NPAD, dtype=dtype)
    lp[:, :ncls] = rnd(a_in.float() @ w3.t())
    r.put("classifier.logits_pad", lp)
    v = lp[:, :ncls].float() + lin3.bias.detach()
    r.put("logits", v)
    lse = torch.logsumexp(v, 1)
    rl = lse - v.gather(1, target.view(-1, 1)).squeeze(1)
    r.put("xent.row_loss", rl)
    rc = (v.argmax(1) == target).float()
    r.put("xent.row_correct", rc)
    r.put("met", torch.stack([rl.mean(), rc.mean()]))
    for n, b in model.named_buffers():
        r.put(f"buf:{n}", b)
    if not train:
        return r
    # ------------------------------------------------------------------------------------------------ backward
    gs = (float(loss_scale) if loss_scale is not None else 1.0) / float(grad_div or N)
    dl = torch.zeros(N, NPAD, dtype=dtype)
    dl[:, :ncls] = rnd((torch.exp(v - lse.view(-1, 1)) - F.one_hot(target, ncls)) * gs)
    r.put("classifier.dlogits", dl)
    grads = {}
    d32 = dl[:, :ncls].float()
    grads[f"classifier.{i3}.bias"] = d32.sum(0)
    grads[f"classifier.{i3}.weight"] = d32.t() @ a_in.float()
    dh32 = d32 @ w3
    if mut == "pad_rows_in_dh":  # padded class rows that are not zero, met by padded dlogits columns that are not zero
        g_ = torch.Generator().manual_seed(3)
        dh32 = dh32 + (torch.exp(-lse) * gs).view(-1, 1) * torch.randn(NPAD - ncls, w3.shape[1], generator=g_).sum(0)
    dh = rnd(dh32)
    r.put(f"classifier.{i3}.dh", dh)
    for i in (1, 0):
        j, lin, dmod = hidden[i]
        Pj = f"classifier.{j}"
        scale = 1.0 if hit("bwd_no_scale", Pj) else pc.dropout_consts(ps[i])[1]
        dz = rnd(torch.where(hs[i] > 0, dh.float() * scale, torch.zeros(())))
        r.put(f"{Pj}.dz", dz)
        grads[f"{Pj}.bias"] = dz.float().sum(0)
        grads[f"{Pj}.weight"] = dz.float().t() @ xins[i].float()
        dh = rnd(dz.float() @ w16(lin))
        r.put(f"{Pj}.dh", dh)
    if drop0 is not None:
        dh = rnd(torch.where(x0 > 0, dh.float() * pc.dropout_consts(pt)[1], torch.zeros(())))
        r.put(f"classifier.{drop0}.dx", dh)
    Cl, hl, wl = fwd[-1]["act"].shape[3], fwd[-1]["act"].shape[1], fwd[-1]["act"].shape[2]
    g = dh.view(N, Cl, hl, wl).permute(0, 2, 3, 1).contiguous()

    def finalize(L, f, sums, rows):
        """(sum dz, sum dz * xhat) [C, 2] in fp64 -> the gradients and, for a BatchNorm, its backward coefficients"""
        P, C = L.path, L.conv.out_channels
        if L.bn is None:
            grads[f"{P}.bias"] = sums[:, 1 if hit("dbias_wrong_column", P) else 0].float()
            return None
        coef = f["coef"]
        mean, invstd = coef[2 * C:3 * C], coef[3 * C:]
        sdz, sdzx = sums[:, 0] * wsz, sums[:, 1] * wsz
        count = rows * wsz
        A = L.bn.weight.detach() * invstd
        mdz, mdzx = (sdz / count).float(), (sdzx / count).float()
        grads[f"{L.bnpath}.weight"], grads[f"{L.bnpath}.bias"] = (sdzx / wsz).float(), (sdz / wsz).float()
        grads[f"{P}.bias"] = sums[:, 0].float() if hit("bias_grad_nonzero", P) else torch.zeros(C)
        bc = torch.cat([A, -A * invstd * mdzx, -A * mdz + A * invstd * mdzx * mean]).contiguous()
        r.put(f"{P}.bcoef", bc)
        return bc

    pending = None  # the backward coefficients of an unpooled layer, finalized with its consumer's backward data
    for li in range(len(layers) - 1, -1, -1):
        L, f = layers[li], fwd[li]
        P, conv = L.path, L.conv
        C = conv.out_channels
        y, coef, act, idx = f["y"], f["coef"], f["act"], f["idx"]
        rows = y.numel() // C
        r.put(f"{P}.g", g)
        if L.pool:
            sc, sh, mean, invstd = coef[:C], coef[C:2 * C], coef[2 * C:3 * C], coef[3 * C:]
            dzp = torch.where(act > 0, g.float(), torch.zeros(()))
            xh = ((act.float() - sh) / sc - mean) * invstd
            sums = torch.stack([dzp.double().reshape(-1, C).sum(0), (dzp * xh).double().reshape(-1, C).sum(0)], 1)
            r.put(f"{P}.slots.0", sums)
            r.meta[f"{P}.slot_chunks"] = [(0, N)]
            bc = finalize(L, f, sums, rows)
            if L.pool == 2:
                dz, _, _ = pc.pool2_bwd_ref(dict(y=y, dp=g, b=None), None, pos=idx, mask=act > 0)
                dz = dz.float()
            else:
                tail = cc.stem_tail_ref(dict(y=y, dp=g, idx=idx, coef=coef, b=torch.zeros(3 * C)), N, y.shape[1], y.shape[2],
                                        C, pad=0)
                dz = torch.where(y.float() * sc + sh > 0, tail["dzraw"].float(), torch.zeros(()))
            dy = rnd(dz) if bc is None else rnd(bc[:C] * dz + bc[C:2 * C] * y.float() + bc[2 * C:])
            r.put(f"{P}.dy", dy)
        elif L.bn is not None:
            bc = pending
            dy = rnd(bc[:C] * g.float() + bc[C:2 * C] * y.float() + bc[2 * C:])
            r.put(f"{P}.dy", dy)
        else:
            dy = g
        # weight gradient, accumulated over the conv's chunks
        ch = chunks_of(li)
        acc = None
        for k, (a, b) in enumerate(ch):
            part = torch.nn.grad.conv2d_weight(_nchw(f["x"][a:b].float()), conv.weight.shape, _nchw(dy[a:b].float()),
                                               conv.stride, conv.padding)
            acc = part if (acc is None or hit("wgrad_chunk2_overwrites", P)) else acc + part
            if len(ch) > 1:
                r.put(f"{P}.wgrad.{k}", acc)
        if len(ch) > 1:
            r.meta[f"{P}.wgrad_chunks"] = ch
        if li == 0:
            R = conv.kernel_size[0]
            if mut == "first_wgrad_rows_swapped":  # the two kernel rows of every pair exchanged (the odd last row stays)
                perm = [r_ ^ 1 if (r_ ^ 1) < R else r_ for r_ in range(R)]
                acc = acc[:, :, perm]
            if mut == "first_wgrad_pad_column":  # columns gathered one to the right: the padding column R kept
                xw = F.pad(_nchw(f["x"].float()), (pad, pad + 1, pad, pad))
                wide = torch.nn.grad.conv2d_weight(xw, (C, 3, R, R + 1), _nchw(dy.float()), conv.stride, 0)
                acc = wide[..., 1:].contiguous()
        grads[f"{P}.weight"] = acc
        if li == 0:
            break
        prev, pf = layers[li - 1], fwd[li - 1]
        xs = f["x"].shape
        d32_ = _nhwc(torch.nn.grad.conv2d_input((xs[0], xs[3], xs[1], xs[2]), w16(conv), _nchw(dy.float()), conv.stride,
                                                conv.padding))
        if prev.pool:
            g = rnd(d32_)
            continue
        yp, cp = pf["y"], pf["coef"]
        Cp = yp.shape[-1]
        dz32 = torch.where(yp.float() * cp[:Cp] + cp[Cp:2 * Cp] > 0, d32_, torch.zeros(()))
        xh = ((yp.float() - cp[2 * Cp:3 * Cp]) * cp[3 * Cp:]).double()
        parts = []
        for k, (a, b) in enumerate(ch):
            d = dz32[a:b].double().reshape(-1, Cp)
            parts.append(torch.stack([d.sum(0), (d * xh[a:b].reshape(-1, Cp)).sum(0)], 1))
            r.put(f"{prev.path}.slots.{k}", parts[-1])
        r.meta[f"{prev.path}.slot_chunks"] = ch
        pending = finalize(prev, pf, parts[0] if hit("slots_chunk2_dropped", prev.path) else sum(parts), yp.numel() // Cp)
        g = rnd(dz32)
    for n, _ in model.named_parameters():
        r.put(f"grad:{n}", grads[n])
    return r


CASES = {"vgg_bias": ("vgg_b", False), "vgg_bn": ("vgg_b", True), "vgg_a_bias": ("vgg_a", False), "vgg_a_bn": ("vgg_a", True),
         "alexnet": ("alexnet", False)}
FULL_RES = {"vgg_a": (0,), "vgg_b": (0, 1), "alexnet": (0,)}  # the convs the chunked step splits (tests/test_vgg_audit_gpu.py)


def _batch(kind, seed, u8=False):
    N, H, W = va.GEOM[kind]
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 256, (N, 3, H, W), generator=g, dtype=torch.uint8) if u8 else torch.randn(N, 3, H, W, generator=g)
    return x, torch.randint(0, va.NCLS, (N,), generator=g)


def _run(case, dtype, train=True, knobs=None, u8=False, loss_scale=None, grad_div=None, world=None, chunked=False, seed=3,
         prev_seeds=()):
    kind, bn = CASES[case]
    model = va.small_model(kind, bn)
    x, t = _batch(kind, seed, u8)
    with torch.no_grad():
        before = {n: b.clone() for n, b in model.named_buffers()}
        rec = emulate_step(model, x, t, dtype, train, knobs, loss_scale, grad_div, world,
                           FULL_RES[kind] if chunked else ())
        found = va.audit(rec, model, before, x, t, dtype, train, loss_scale, grad_div, world, family="vggstep_cpu",
                         prev_seeds=prev_seeds)
    return model, rec, found


def _complete(model, rec, train=True):
    if train:
        for n, _ in model.named_parameters():
            assert f"grad:{n}" in rec.judged, n
    for n, _ in model.named_buffers():
        assert f"buf:{n}" in rec.judged, n
    assert set(rec.t) <= set(rec.judged)
    assert max(rec.judged.values()) <= 1.0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("chunked", [False, True])
@pytest.mark.parametrize("case", sorted(CASES))
def test_emulated_step_passes_the_audit_and_is_judged_completely(case, chunked, dtype):
    model, rec, found = _run(case, dtype, chunked=chunked)
    assert not found, va.report(found)
    _complete(model, rec)
    if chunked:
        assert any(k.endswith(".wgrad.1") for k in rec.t)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", ["vgg_bias", "vgg_bn", "alexnet"])
def test_emulated_eval_step_passes(case, dtype):
    model, rec, found = _run(case, dtype, train=False)
    assert not found, va.report(found)
    _complete(model, rec, train=False)
    assert all(p == 0.0 for p, _ in rec.meta["dropout"].values())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", sorted(CASES))
def test_undecided_masks_stay_under_the_cap_on_the_reference_alone(case, dtype):
    """The share of elements whose ReLU branch fp32 may call either way, from the record's y and coef alone, for every
    unpooled layer (fused mask) and every MaxPool(3, 2) layer (gather backward): the seeds the tests use keep it under
    MASK_CAP."""
    model, rec, _ = _run(case, dtype)
    n = 0
    for L in va.feature_layers(model):
        if L.pool != 2:
            y, coef = rec.t[f"{L.path}.y"], rec.t[f"{L.path}.coef"]
            _, unsure = sa.pre_mask(y, coef, y.shape[-1])
            assert float(unsure.double().mean()) <= sa.MASK_CAP, L.path
            n += 1
    assert n >= 1


def test_uint8_loss_scale_and_world_pass():
    for case, kw in (("vgg_bias", dict(u8=True)), ("alexnet", dict(loss_scale=1024.0, grad_div=6.0)),
                     ("vgg_bn", dict(loss_scale=1024.0, grad_div=6.0)), ("vgg_bn", dict(world=2)),
                     ("vgg_a_bn", dict(world=2, chunked=True)), ("vgg_bn", dict(world=1))):
        _, _, found = _run(case, torch.float16, **kw)
        assert not found, (case, kw, va.report(found))


def test_dropout_seeds_of_the_previous_step_are_refused():
    _, rec, found = _run("vgg_bias", torch.bfloat16)
    assert not found
    seeds = [s for _, s in rec.meta["dropout"].values()]
    _, _, found = _run("vgg_bias", torch.bfloat16, prev_seeds=seeds[:1])
    assert [(f.path, f.quantity) for f in found] == [("classifier", "dropout seeds")], va.report(found)


def test_executor_seed_stride_keeps_the_launches_of_any_two_steps_apart():
    """VGGExecutor draws with seed + 0, seed + 1 (hidden layers) and seed + 7 (AlexNet's feature dropout) and advances
    the seed by ``_DROP_STRIDE`` per step: no difference of two offsets may be a multiple of the stride."""
    from pytorch_distributed_template_amd.models.executor_vgg import VGGExecutor
    stride = VGGExecutor._DROP_STRIDE
    offsets = (0, 1, 7)
    seen = set()
    for step in range(1, 4097):
        now = {stride * step + o for o in offsets}
        assert len(now) == len(offsets) and not (now & seen), step
        seen |= now


# mutation -> (case, knobs, extra _run arguments, {path: words one of which the quantity must contain}).  What teacher
# forcing allows besides the mutated quantity:
#  * a wrong coef (count, dropped chunk statistics) is judged at its BatchNorm only; so are the running mean and the eval
#    shift without their bias term;
#  * dropped fused slots of a chunk move dgamma / dbeta / bcoef of the producer's BatchNorm (the recorded chunk sums are
#    right: the finalize read the wrong total);
#  * an overwriting weight-gradient chunk shows in the final gradient and in the recorded prefix after chunk 2;
#  * a second hidden layer of AlexNet given dropout: its h, and the dz that the reference forms without the scale;
#  * a shared seed is a finding of its own: every h is judged with its recorded seed.
MUTATIONS = {
    "rm_no_bias": ("vgg_bn", dict(at="features.3"), {}, {"features.4": ["coef / running statistics"]}),
    "eval_no_bias": ("vgg_bn", dict(at="features.7"), dict(train=False), {"features.8": ["coef / running statistics"]}),
    "bias_grad_nonzero": ("vgg_bn", dict(at="features.3"), {}, {"features.3": ["bias gradient"]}),
    "count_plus_image": ("vgg_bn", dict(at="features.10"), {}, {"features.11": ["coef"]}),
    "stats_chunk2_dropped": ("vgg_bn", dict(at="features.3"), dict(chunked=True), {"features.4": ["coef"]}),
    "wgrad_chunk2_overwrites": ("vgg_bias", dict(at="features.2"), dict(chunked=True), {"features.2": ["weight gradient"]}),
    "slots_chunk2_dropped": ("vgg_bn", dict(at="features.0"), dict(chunked=True), {"features.1": ["dgamma"]}),
    "first_wgrad_rows_swapped": ("alexnet", {}, {}, {"features.0": ["weight gradient"]}),
    "first_wgrad_pad_column": ("alexnet", {}, {}, {"features.0": ["weight gradient"]}),
    "flatten_nhwc": ("vgg_bias", {}, {}, {"classifier": ["flattened features"]}),
    "same_seed": ("vgg_bias", dict(at="classifier.3"), {}, {"classifier": ["dropout seeds"]}),
    "bwd_no_scale": ("vgg_bias", dict(at="classifier.0"), {}, {"classifier.0": ["dz"]}),
    "h2_dropout": ("alexnet", dict(at="classifier.4"), {}, {"classifier.4": ["h (bias", "dz"]}),
    "pad_rows_in_dh": ("vgg_bias", {}, {}, {"classifier.6": ["dh"]}),
    "dbias_wrong_column": ("vgg_bias", dict(at="features.2"), {}, {"features.2": ["dbias"]}),
}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mut", sorted(MUTATIONS))
def test_each_wiring_mutation_is_found_at_its_layer(mut, dtype):
    case, knobs, kw, allowed = MUTATIONS[mut]
    _, _, found = _run(case, dtype, knobs=dict(knobs, mut=mut), **kw)
    assert found, f"{mut}: the audit found nothing"
    first = next(iter(allowed))
    assert any(f.path == first and any(w in f.quantity for w in allowed[first]) for f in found), va.report(found)
    stray = [f for f in found if not (f.path in allowed and any(w in f.quantity for w in allowed[f.path]))]
    assert not stray, f"{mut}: findings outside the mutated layer:\n" + va.report(stray)


def test_mutations_on_the_other_routes_of_the_bias_sums():
    """The same wiring errors where the routes differ: the dropped fused slots under a bias layer (dbias), and dbias from
    the wrong column at a POOLED bias layer."""
    for case, knobs, kw, allowed in (
            ("vgg_bias", dict(mut="slots_chunk2_dropped", at="features.0"), dict(chunked=True), {"features.0": ["dbias"]}),
            ("vgg_a_bias", dict(mut="dbias_wrong_column", at="features.0"), {}, {"features.0": ["dbias"]})):
        _, _, found = _run(case, torch.bfloat16, knobs=knobs, **kw)
        assert found and all(f.path in allowed and any(w in f.quantity for w in allowed[f.path]) for f in found), \
            (case, knobs, va.report(found))
