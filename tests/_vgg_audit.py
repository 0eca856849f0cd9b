"""Teacher-forced audit of one VGGExecutor step -- VGG, VGG-BN, AlexNet (a plain module, not a conftest).

The same two halves as tests/_step_audit.py, whose ``Finding``, ``StepRecord``, ``_masked_compare``, ``report`` and
``MASK_CAP`` it reuses:

``extract_record`` turns what a step left behind -- ``saved``, the executor's work buffers and the ``Tape`` of its
launches (tests/_tape.py) -- into a ``StepRecord`` of plain named tensors in logical layout.  It is the only part that
knows buffer keys and tape positions.  Names follow the module tree; ``<c>`` is the index of a conv in ``features``,
``<l>`` of a Linear (or the leading Dropout) in ``classifier``:

* ``input.packed``; ``features.<c>.y`` / ``.coef`` / ``.act`` (the layer's output activation, pooled where a max-pool
  follows) / ``.idx`` / ``.g`` (gradient of ``act``) / ``.dy`` (conv-output gradient, absent where it IS ``g``: an
  unpooled bias layer) / ``.bcoef`` (BatchNorm layers);
* per launch chunk k (k = 0 alone when the launch is not split; ``meta["features.<c>.chunks"]`` etc. hold the image
  ranges): ``features.<c>.stats.<k>`` (forward statistics [C, 2]), ``features.<c>.slots.<k>`` (BN-backward sums [C, 2]
  of the pooled reduce or of the consumer's fused backward-data epilogue) and, for a split weight gradient,
  ``features.<c>.wgrad.<k>`` (the gradient as ``wgrad_reduce`` left it after chunk k);
* ``classifier.featc``, ``classifier.<l>.x`` (AlexNet's feature dropout), ``classifier.<l>.z`` / ``.h`` / ``.dz`` /
  ``.dh`` (``dh``: the gradient of the Linear's INPUT), ``classifier.<l>.dx`` (feature dropout backward),
  ``classifier.logits_pad`` / ``.dlogits``; ``logits``, ``xent.*``, ``met``; ``grad:<param>``; ``buf:<buffer>``;
* ``meta["dropout"]``: {name: (p, seed)} of every ``fc_act_fwd`` launch.

``audit`` judges EVERY recorded tensor per element against fp64, each reference computed from the record's own upstream
tensors, the parameters in logical torch layout (``.to(dtype).double()``; biases and BatchNorm parameters are read in
fp32) and the buffers snapshotted before the step.  It never reads the shadow, the derived layouts, the index maps or
``first_conv_maps``.  The bounds are those of tests/_numerics.py and tests/_pool_cases.py, unchanged:

* convs (the first included: F.conv2d semantics on the packed image's logical content) ``conv_bound``; forward statistics
  ``assert_conv_stats`` per chunk; training finalize ``finalize_carried`` / ``check_finalize_carried``; fused backward sums
  the ``assert_bnb_sums`` bounds per chunk, carried into ``check_bwd_finalize_carried``; pools ``assert_pool_fwd``,
  ``pool2_bwd_ref``, ``assert_pooled_link``, ``assert_pool_bwd``; dropout ``fc_act_ref`` / ``fc_act_bwd_ref`` bit for bit
  with the keep mask of ``vgg_hash_torch`` at the recorded seed; loss ``xent_ref``;
* the Linear GEMMs accumulate in fp32 and round once: ``conv_bound`` with n = the reduction length (z, logits, dh);
  their weight gradients are the conv weight-gradient kernel: the weight-gradient bound with n = N.

Departures of the executor from autograd, encoded instead of tolerated:

* a conv bias in front of a BatchNorm never reaches a kernel.  Its gradient is EXACTLY zero; the running mean gains
  ``momentum * bias`` in one more fp32 multiply-add (2 roundings on top of the finalize's, inside the same
  ``6u * sum|term|`` with ``|momentum * bias|`` as a third term); the eval shift gains ``scale * bias`` (``addcmul_``: 2
  roundings, inside ``10u * sum|term|`` with ``|scale * bias|`` as a third term);
* a bias layer is a BatchNorm with coefficients EXACTLY ``[1 | bias | 0 | 1]``; its ``dbias`` is the ``sum dz`` reference;
* ``num_batches_tracked`` is untouched;
* the seeds of all dropout launches of a step are distinct and differ from the previous step's (``prev_seeds``); the
  dropout probability of every launch is the one the module tree asks for (AlexNet's second hidden layer: none).

Undecided ReLU elements are handled as in tests/_step_audit.py: left out of the element comparison, counted whole in the
sums' bounds, at most ``MASK_CAP`` of a tensor.
"""
from collections import namedtuple

import math

import torch
import torch.nn as nn

import _conv_cases as cc
import _numerics as nm
import _pool_cases as pc
import _step_audit as sa
from _numerics import U
from _step_audit import MASK_CAP, Finding, StepRecord, _exact, _masked_compare, report  # noqa: F401

FLayer = namedtuple("FLayer", "path conv bnpath bn pool")


def feature_layers(model):
    """[FLayer] of ``model.features``: conv (+ BatchNorm) + ReLU (+ MaxPool: ``pool`` = its kernel size, else 0)."""
    mods = list(model.features)
    out, i = [], 0
    while i < len(mods):
        ci, conv = i, mods[i]
        assert isinstance(conv, nn.Conv2d), conv
        i += 1
        bi = bn = None
        if isinstance(mods[i], nn.BatchNorm2d):
            bi, bn = i, mods[i]
            i += 1
        assert isinstance(mods[i], nn.ReLU), mods[i]
        i += 1
        pool = 0
        if i < len(mods) and isinstance(mods[i], nn.MaxPool2d):
            k = mods[i].kernel_size
            pool = k if isinstance(k, int) else k[0]
            i += 1
        out.append(FLayer(f"features.{ci}", conv, None if bn is None else f"features.{bi}", bn, pool))
    return out


def classifier_plan(model):
    """(index of a leading Dropout or None, [(index, Linear, the Dropout right behind its ReLU or None)] of the hidden
    layers, (index, last Linear))."""
    mods = list(model.classifier)
    lin = [(i, m) for i, m in enumerate(mods) if isinstance(m, nn.Linear)]
    hidden = [(i, m, mods[i + 2] if i + 2 < len(mods) and isinstance(mods[i + 2], nn.Dropout) else None)
              for i, m in lin[:-1]]
    return (0 if isinstance(mods[0], nn.Dropout) else None), hidden, lin[-1]


# ====================================================================================================== small models
CFGS = {"vgg_a": [64, "M", 128, "M", 256, 256, "M"],   # pooled first conv, one unpooled -> pooled pair, 256 channels
        "vgg_b": [64, 64, "M", 128, 128, "M"]}         # unpooled first conv feeding a fused-mask backward data
GEOM = {"vgg_a": (3, 32, 64), "vgg_b": (3, 32, 64), "alexnet": (3, 101, 133)}  # N, H, W
FINAL = {"vgg_a": (256, 4, 8), "vgg_b": (128, 8, 16), "alexnet": (256, 2, 3)}   # C, h, w of the last pooled map
HIDDEN, NCLS = 128, 10


def small_model(kind, bn=False, seed=0, p=0.5):
    """A VGG (``kind`` of CFGS, with BatchNorm or bias) or AlexNet (stock ``features``) instance with a small classifier
    -- three Linears, hidden 128, 10 classes, the family's Dropout order --, built without the stock 25088 x 4096 one;
    every BatchNorm its own eps and momentum, BatchNorm parameters, running statistics and all biases randomised."""
    from pytorch_distributed_template_amd.models.classic import VGG, AlexNet, make_vgg_layers
    torch.manual_seed(seed)
    C, h, w = FINAL[kind]
    feat = C * h * w
    lin = [nn.Linear(feat, HIDDEN), nn.Linear(HIDDEN, HIDDEN), nn.Linear(HIDDEN, NCLS)]
    if kind == "alexnet":
        m = AlexNet.__new__(AlexNet)
        nn.Module.__init__(m)
        m.features = nn.Sequential(
            nn.Conv2d(3, 64, kernel_size=11, stride=4, padding=2), nn.ReLU(inplace=True), nn.MaxPool2d(kernel_size=3, stride=2),
            nn.Conv2d(64, 192, kernel_size=5, padding=2), nn.ReLU(inplace=True), nn.MaxPool2d(kernel_size=3, stride=2),
            nn.Conv2d(192, 384, kernel_size=3, padding=1), nn.ReLU(inplace=True),
            nn.Conv2d(384, 256, kernel_size=3, padding=1), nn.ReLU(inplace=True),
            nn.Conv2d(256, 256, kernel_size=3, padding=1), nn.ReLU(inplace=True), nn.MaxPool2d(kernel_size=3, stride=2))
        m.classifier = nn.Sequential(nn.Dropout(p), lin[0], nn.ReLU(True), nn.Dropout(p), lin[1], nn.ReLU(True), lin[2])
    else:
        m = VGG.__new__(VGG)
        nn.Module.__init__(m)
        m.features = make_vgg_layers(CFGS[kind], batch_norm=bn)
        m.classifier = nn.Sequential(lin[0], nn.ReLU(True), nn.Dropout(p), lin[1], nn.ReLU(True), nn.Dropout(p), lin[2])
    m.avgpool = nn.AdaptiveAvgPool2d((h, w))
    k = 0
    for mod in m.modules():
        if isinstance(mod, nn.BatchNorm2d):
            mod.weight.data.uniform_(0.5, 1.5)
            mod.bias.data.uniform_(-0.2, 0.2)
            mod.running_mean.uniform_(-0.5, 0.5)
            mod.running_var.uniform_(0.5, 1.5)
            mod.eps = (1e-5, 1e-4, 1e-3)[k % 3]
            mod.momentum = (1.0, 0.999, 0.998, 0.997)[k % 4]
            k += 1
        if isinstance(mod, (nn.Conv2d, nn.Linear)):
            mod.bias.data.uniform_(-0.3, 0.3)
    return m


# ====================================================================================================== extraction
def _slot_sums(t, C):
    return t.view(-1, C, 2).sum(0)


def extract_record(ex, saved, tape, model, train):
    """StepRecord of the step that produced ``saved`` (the return value of ``ex._forward``) and ``tape``."""
    r = StepRecord(train)
    N = saved["N"]
    es = 2  # bytes of a 16-bit element
    layers = feature_layers(model)
    assert len(layers) == len(ex.layers)
    buf = lambda key, dt=None: ex._bufs[(key, dt or ex.dtype)]
    inside = lambda a, t, size: torch.is_tensor(a) and t.data_ptr() <= a.data_ptr() < t.data_ptr() + t.numel() * size

    def chunks_of(calls, pos, base, per_image, n_of):
        """Image ranges of the launches ``calls`` from where their argument ``pos`` starts inside ``base``."""
        out = []
        for c in calls:
            a = (c.args[pos].data_ptr() - base.data_ptr()) // (per_image * es)
            out.append((a, a + n_of(c)))
        return out

    r.put("input.packed", tape.named("stem_pack", "stem_pack_u8")[-1].outs[1].view(N, saved["Hp"], saved["Wp"], 4))
    dims = []
    for li, (L, E) in enumerate(zip(layers, ex.layers)):
        x, h, w, y, out, idx = saved["acts"][li]
        C = L.conv.out_channels
        P = L.path
        r.put(f"{P}.y", y.view(N, h, w, C))
        r.put(f"{P}.coef", E.coef)
        fw = sorted((c for c in tape.named("conv_fwd") if inside(c.args[2], y, es)), key=lambda c: c.args[2].data_ptr())
        r.meta[f"{P}.chunks"] = chunks_of(fw, 2, y, h * w * C, lambda c: c.args[5])
        for k, c in enumerate(fw):
            if 4 in c.outs:
                r.put(f"{P}.stats.{k}", _slot_sums(c.outs[4], C))
        ho, wo = (h, w) if not L.pool else ((h // 2, w // 2) if L.pool == 2 else ((h - 3) // 2 + 1, (w - 3) // 2 + 1))
        r.put(f"{P}.act", out.view(N, ho, wo, C))
        if idx is not None:
            r.put(f"{P}.idx", idx.view(N, ho, wo, C))
        dims.append((h, w, ho, wo, C))
    r.put("classifier.featc", saved["featc"].view(N, ex.feat))
    drop0, hidden, (i3, _) = classifier_plan(model)
    names = {}
    if saved["x0"] is not None:
        r.put(f"classifier.{drop0}.x", saved["x0"].view(N, ex.feat))
        names[saved["x0"].data_ptr()] = f"classifier.{drop0}"
    for i, (j, lin, _) in enumerate(hidden):
        r.put(f"classifier.{j}.z", buf(("fcz", i)).view(N, lin.out_features))
        r.put(f"classifier.{j}.h", saved["hs"][i].view(N, lin.out_features))
        names[saved["hs"][i].data_ptr()] = f"classifier.{j}"
    r.meta["dropout"] = {names[c.args[2].data_ptr()]: (float(c.args[5]), int(c.args[6])) for c in tape.named("fc_act_fwd")}
    r.put("classifier.logits_pad", saved["logits"].view(N, ex.ncls_pad))
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
    r.put("classifier.dlogits", xe.outs[7].view(N, ex.ncls_pad))
    r.put(f"classifier.{i3}.dh", buf(("fcdh", 1)).view(N, ex.hidden))
    for i, (j, lin, _) in enumerate(hidden):
        r.put(f"classifier.{j}.dz", buf(("fcdz", i)).view(N, lin.out_features))
        r.put(f"classifier.{j}.dh", buf(("fcdh", i - 1) if i > 0 else "dfeatc").view(N, lin.in_features))
    if saved["x0"] is not None:
        r.put(f"classifier.{drop0}.dx", buf("dfeat0").view(N, ex.feat))
    for li in range(len(layers) - 1, -1, -1):
        L, E = layers[li], ex.layers[li]
        h, w, ho, wo, C = dims[li]
        P = L.path
        y = saved["acts"][li][3]
        g = buf("g_pool") if li == len(layers) - 1 else buf(("g", li))
        r.put(f"{P}.g", g.view(N, ho, wo, C))
        if L.pool or L.bn is not None:
            r.put(f"{P}.dy", buf(("dy", li)).view(N, h, w, C))
        if L.bn is not None:
            r.put(f"{P}.bcoef", E.bcoef)
        if L.pool:
            pr = [c for c in tape.named("pooled_bwd_reduce") if c.args[1].data_ptr() == saved["acts"][li][4].data_ptr()]
            assert len(pr) == 1, f"{P}: {len(pr)} pooled reduces"
            r.put(f"{P}.slots.0", _slot_sums(pr[0].outs[3], C))
            r.meta[f"{P}.slot_chunks"] = [(0, N)]
        else:
            dg = sorted((c for c in tape.named("conv_dgrad_bn") if inside(c.args[17], y, es)),
                        key=lambda c: c.args[17].data_ptr())
            assert dg, f"{P}: no fused backward-data launch reads this layer's conv output"
            r.meta[f"{P}.slot_chunks"] = chunks_of(dg, 17, y, h * w * C, lambda c: c.args[4])
            for k, c in enumerate(dg):
                r.put(f"{P}.slots.{k}", _slot_sums(c.outs[22], C))
        # a weight gradient split over image chunks: what wgrad_reduce left after every chunk, in logical layout
        K, Ci, R, S = L.conv.weight.shape
        if li == 0:
            tmp = ex._bufs.get(("w0_dw", torch.float32))
            wr = [c for c in tape.named("wgrad_reduce") if tmp is not None and c.args[6].data_ptr() == tmp.data_ptr()]
            logical = lambda t: t.reshape(-1)[ex.w0_gidx.long()].view(K, R, S, Ci).permute(0, 3, 1, 2)
            span = max(saved["Hp"] * saved["Wp"] * 4, h * w * C)
        else:
            gv = ex._g(E.conv.slot)
            wr = [c for c in tape.named("wgrad_reduce") if c.args[6].data_ptr() == gv.data_ptr()]
            logical = lambda t: t.view(K, R, S, Ci).permute(0, 3, 1, 2)
            hin, win = dims[li - 1][2], dims[li - 1][3]
            span = hin * win * max(Ci, K)
        if len(wr) > 1:
            ch = ex._chunks(N, span)
            assert len(ch) == len(wr), f"{P}: {len(wr)} weight-gradient reduces over {len(ch)} chunks"
            r.meta[f"{P}.wgrad_chunks"] = ch
            for k, c in enumerate(wr):
                r.put(f"{P}.wgrad.{k}", logical(c.outs[6]))
    for n, p in model.named_parameters():
        r.put(f"grad:{n}", p.grad)
    return r


# ====================================================================================================== the walk
def audit(record, model, buffers_before, images, target, dtype, train=True, loss_scale=None, grad_div=None,
          syncbn_world=None, family="vggstep", prev_seeds=()):
    """Judge every tensor of ``record``; returns the list of Findings (empty: the step is right).  Arguments as
    ``_step_audit.audit``; ``prev_seeds``: the dropout seeds of the previous step."""
    rec = record
    wk = sa._Walk(rec, model, dtype, family)
    t, judge, fam = wk.t, wk.judge, wk.family
    dev = t("input.packed").device
    world = int(syncbn_world) if syncbn_world else 1
    N = images.shape[0]
    f64 = lambda v: v.detach().to(dev).double()
    f32 = lambda v: v.detach().to(dev).float()
    zero = torch.zeros((), dtype=torch.float64, device=dev)
    layers = feature_layers(model)

    def chunk_names(P, kind, meta):
        ch = rec.meta[f"{P}.{meta}"]
        names = [f"{P}.{kind}.{k}" for k in range(len(ch))]
        assert ch[0][0] == 0 and ch[-1][1] == N and all(a[1] == b[0] for a, b in zip(ch, ch[1:])), \
            f"{P}: the {kind} launches cover the images {ch}, not 0..{N}"
        return list(zip(names, ch))

    # ---------------------------------------------------------------------------------------------- the pack
    c0 = layers[0].conv
    pad = c0.padding[0]
    H, W = images.shape[2], images.shape[3]
    xp = t("input.packed")
    if images.dtype == torch.uint8:
        from pytorch_distributed_template_amd.data.transforms import IMAGENET_MEAN, IMAGENET_STD
        mean = torch.tensor(IMAGENET_MEAN, dtype=torch.float64, device=dev).view(1, 3, 1, 1)
        std = torch.tensor(IMAGENET_STD, dtype=torch.float64, device=dev).view(1, 3, 1, 1)
        xd = images.to(dev).double()
        img_ref, img_mag = (xd / 255.0 - mean) / std, (xd / (255.0 * std)).abs() + (mean / std).abs()
    else:
        img_ref, img_mag = images.to(dev).float().to(dtype).double(), None  # a cast: exact

    def packed():
        # the zero border and the spare rows / columns behind it included
        assert xp.shape[1] >= H + 2 * pad and xp.shape[2] >= W + 2 * pad and xp.shape[3] == 4
        exp = torch.zeros(xp.shape, dtype=torch.float64, device=dev)
        exp[:, pad:pad + H, pad:pad + W, :3] = img_ref.permute(0, 2, 3, 1)
        if img_mag is None:
            return _exact(xp, exp, "packed image")
        border = torch.ones(xp.shape, dtype=torch.bool, device=dev)
        border[:, pad:pad + H, pad:pad + W, :3] = False
        _exact(xp[border], exp[border], "packed image: border, spare rows and fourth channel")
        mg = torch.zeros_like(exp)
        mg[:, pad:pad + H, pad:pad + W, :3] = img_mag.permute(0, 2, 3, 1)
        return nm.assert_rounded(xp, exp, mg, dtype, 8, "packed image", 4, fam("pack_u8"))
    judge("input.packed", layers[0].path, "packed image", packed)
    x_img = xp[:, pad:pad + H, pad:pad + W, :3].contiguous()

    # ---------------------------------------------------------------------------------------------- features forward
    def coef_check(L, y, coef):
        C = L.conv.out_channels
        P = L.path
        bias = None if L.conv.bias is None else f32(L.conv.bias)
        if L.bn is None:
            def run():
                exp = torch.cat([torch.ones(C, device=dev), bias, torch.zeros(C, device=dev), torch.ones(C, device=dev)])
                return _exact(coef, exp, f"{P}: bias coefficients [1 | bias | 0 | 1]")
            judge(f"{P}.coef", P, "coef (bias)", run)
            return
        bn, bp = L.bn, L.bnpath
        rm0, rv0 = buffers_before[f"{bp}.running_mean"].to(dev), buffers_before[f"{bp}.running_var"].to(dev)
        names = [f"{P}.coef", f"buf:{bp}.running_mean", f"buf:{bp}.running_var", f"buf:{bp}.num_batches_tracked"]
        b64 = torch.zeros(C, dtype=torch.float64, device=dev) if bias is None else bias.double()

        def run():
            rm, rv = t(f"buf:{bp}.running_mean"), t(f"buf:{bp}.running_var")
            _exact(t(f"buf:{bp}.num_batches_tracked"), buffers_before[f"{bp}.num_batches_tracked"].to(dev),
                   f"{bp}: num_batches_tracked")
            if not train:
                _exact(rm, rm0, f"{bp}: running_mean (eval)")
                _exact(rv, rv0, f"{bp}: running_var (eval)")
                eps32 = float(torch.tensor(bn.eps, dtype=torch.float32))
                invstd = 1.0 / torch.sqrt(rv0.double() + eps32)
                scale = f64(bn.weight) * invstd
                shift = f64(bn.bias) - rm0.double() * scale + scale * b64  # the conv bias enters the eval shift only
                fm = fam("eval_coef")
                w = nm.assert_within(coef[3 * C:], invstd, 8 * U * invstd.abs(), f"{bp}: eval invstd", C, fm)
                w = max(w, nm.assert_within(coef[:C], scale, 8 * U * scale.abs(), f"{bp}: eval scale", C, fm))
                w = max(w, nm.assert_within(coef[C:2 * C], shift, 10 * U * (
                    f64(bn.bias).abs() + (rm0.double() * scale).abs() + (scale * b64).abs()), f"{bp}: eval shift", C, fm))
                _exact(coef[2 * C:3 * C], rm0, f"{bp}: eval mean")
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
            fm = fam("finalize")
            w = nm.check_finalize_carried(coef, None, None, ref, car, C, bp, fm)
            # the running statistics by check_finalize_carried's formulas, the running mean with its bias term
            mom32 = float(torch.tensor(mom, dtype=torch.float32))
            mb = mom32 * b64
            w = max(w, nm.assert_within(rm, ref["rm_old"] + ref["rm_new"] + mb, car["rm"] + 6 * U * (
                ref["rm_old"].abs() + ref["rm_new"].abs() + mb.abs() + car["rm"]), f"{bp}: running_mean", C, fm))
            w = max(w, nm.assert_within(rv, ref["rv_old"] + ref["rv_new"], car["rv"] + 6 * U * (
                ref["rv_old"].abs() + ref["rv_new"].abs() + car["rv"]), f"{bp}: running_var", C, fm))
            return w
        judge(names, bp, "coef / running statistics", run)

    x = x_img
    for L in layers:
        P, conv = L.path, L.conv
        C = conv.out_channels
        y, coef = t(f"{P}.y"), t(f"{P}.coef")

        def conv_run(x=x, conv=conv, P=P):
            ref, mag = nm.conv_fwd_ref(x, sa.krsc(conv, dtype), conv.stride[0], conv.padding[0])
            n = conv.kernel_size[0] * conv.kernel_size[1] * conv.in_channels
            return nm.assert_conv(t(f"{P}.y"), ref, mag, n, dtype, f"{P}: y", fam("conv_fwd"))
        judge(f"{P}.y", P, "y", conv_run)
        have_stats = rec.has(f"{P}.stats.0")
        assert have_stats == (train and L.bn is not None), f"{P}: forward statistics recorded: {have_stats}"
        if have_stats:
            for name, (a, b) in chunk_names(P, "stats", "chunks"):
                judge(name, P, f"forward statistics of images {a}..{b}", lambda name=name, a=a, b=b, y=y: nm.assert_conv_stats(
                    t(name)[:, 0], t(name)[:, 1], y[a:b], name, fam("conv_stats")))
        coef_check(L, y, coef)
        act = t(f"{P}.act")
        if L.pool:
            k, dead = (2, None) if L.pool == 2 else (3, 255)
            has_idx = rec.has(f"{P}.idx")
            assert has_idx == (train or k == 3), f"{P}: argmax recorded: {has_idx}"

            def pool_run(y=y, coef=coef, act=act, k=k, dead=dead, P=P, has_idx=has_idx):
                rr = pc.pool_fwd_ref(y, coef, k, 0)
                return pc.assert_pool_fwd(act, t(f"{P}.idx") if has_idx else None, rr, dtype, dead, f"{P}: pool", fam("pool"))
            judge([f"{P}.act"] + ([f"{P}.idx"] if has_idx else []), P, "act / argmax (pooled)", pool_run)
        else:
            def act_run(y=y, coef=coef, act=act, C=C, P=P):
                _, ref, mag = nm.bn_apply_ref(y, coef, None, None, C, 0, True)
                return nm.assert_rounded(act.reshape(-1, C), ref, mag, dtype, 8, f"{P}: act", C, fam("apply"))
            judge(f"{P}.act", P, "act", act_run)
        x = act

    # ---------------------------------------------------------------------------------------------- classifier
    drop0, hidden, (i3, lin3) = classifier_plan(model)
    dropout = rec.meta["dropout"]
    feat = t("classifier.featc")
    F_ = feat.shape[1]

    def keep_of(name, p, n):
        if p <= 0.0:
            return None
        thr, _ = pc.dropout_consts(p)
        return pc.vgg_hash_torch(dropout[name][1], n, 0, dev) >= thr

    def want_p(name, mod):
        """The launch's dropout probability is the module tree's (0 in eval, 0 where no Dropout follows)."""
        p = float(mod.p) if (train and mod is not None) else 0.0
        assert name in dropout, f"{name}: no bias + ReLU + dropout launch recorded"
        assert dropout[name][0] == p, f"{name}: dropout p = {dropout[name][0]} launched, the model asks for {p}"
        return p

    def seeds():
        sd = [s for _, s in dropout.values()]
        assert len(set(sd)) == len(sd), f"dropout launches share a seed: {dropout}"
        again = sorted(set(sd) & set(prev_seeds))
        assert not again, f"dropout seeds of the previous step used again: {again}"
        want = {f"classifier.{j}" for j, _, _ in hidden} | ({f"classifier.{drop0}"} if drop0 is not None else set())
        assert set(dropout) == want, f"dropout launches {sorted(dropout)}, expected {sorted(want)}"
        return 0.0
    judge([], "classifier", "dropout seeds", seeds)
    judge("classifier.featc", "classifier", "flattened features (NCHW order)",
          lambda: _exact(feat, x.permute(0, 3, 1, 2).reshape(N, -1), "classifier input"))
    a_in = feat
    if drop0 is not None:
        nx = f"classifier.{drop0}.x"

        def x0_run():
            p = want_p(f"classifier.{drop0}", model.classifier[drop0])
            ref = pc.fc_act_ref(feat, torch.zeros(F_, device=dev), F_, p, keep_of(f"classifier.{drop0}", p, N * F_), dtype)
            return nm.assert_exact(t(nx), ref, nx)
        judge(nx, f"classifier.{drop0}", "feature dropout", x0_run)
        a_in = t(nx)
    lin_in = {}
    for j, lin, dmod in hidden:
        Pj = f"classifier.{j}"
        lin_in[j] = a_in
        wj = lin.weight.detach().to(dev).to(dtype).double()

        def z_run(a_in=a_in, wj=wj, lin=lin, Pj=Pj):
            a64 = a_in.double()
            ref, mag = a64 @ wj.t(), a64.abs() @ wj.abs().t()
            return nm.assert_within(t(f"{Pj}.z"), ref, nm.conv_bound(ref, mag, lin.in_features, dtype), f"{Pj}: z",
                                    lin.out_features, fam("linear"), ref.shape)
        judge(f"{Pj}.z", Pj, "z", z_run)

        def h_run(lin=lin, dmod=dmod, Pj=Pj):
            p = want_p(Pj, dmod)
            Fo = lin.out_features
            ref = pc.fc_act_ref(t(f"{Pj}.z"), f32(lin.bias), Fo, p, keep_of(Pj, p, N * Fo), dtype)
            return nm.assert_exact(t(f"{Pj}.h"), ref, f"{Pj}: h")
        judge(f"{Pj}.h", Pj, "h (bias + ReLU + dropout)", h_run)
        a_in = t(f"{Pj}.h")
    lin_in[i3] = a_in
    ncls, hid = lin3.out_features, lin3.in_features
    w3 = lin3.weight.detach().to(dev).to(dtype).double()
    lp = t("classifier.logits_pad")
    P3 = f"classifier.{i3}"

    def logits_pad():
        a64 = a_in.double()
        ref, mag = a64 @ w3.t(), a64.abs() @ w3.abs().t()
        _exact(lp[:, ncls:], torch.zeros_like(lp[:, ncls:]), "padded class columns")  # no bias in this buffer
        return nm.assert_within(lp[:, :ncls], ref, nm.conv_bound(ref, mag, hid, dtype), "logits", ncls, fam("linear"), ref.shape)
    judge("classifier.logits_pad", P3, "logits (padded, no bias)", logits_pad)
    gs = (float(loss_scale) if loss_scale is not None else 1.0) / float(grad_div or N)
    xr = nm.xent_ref(lp, lin3.bias.detach().to(dev), target.to(dev), ncls, gs, dtype)

    def xent():
        w = nm.assert_rounded(t("logits"), xr["v"], xr["vmag"], torch.float32, 1, "returned logits", ncls, fam("xent"))
        w = max(w, nm.assert_within(t("xent.row_loss"), xr["loss"], xr["loss_bound"], "row loss", None, fam("xent")))
        _exact(t("xent.row_correct"), xr["correct"], "row correct")
        return w
    judge(["logits", "xent.row_loss", "xent.row_correct"], P3, "returned logits / loss / correct", xent)

    def met():
        rl, rc = t("xent.row_loss").double(), t("xent.row_correct").double()
        ref = torch.stack([rl.mean(), rc.mean()])
        return nm.assert_sum(t("met"), ref, torch.stack([rl.abs().mean(), rc.mean()]), math.ceil(N / 256) + 9, "met", 2,
                             fam("xent"))
    judge("met", P3, "met", met)
    if not train:
        return sa._finish(wk)

    # ---------------------------------------------------------------------------------------------- classifier backward
    dl = t("classifier.dlogits")

    def dlogits():
        _exact(dl[:, ncls:], torch.zeros_like(dl[:, ncls:]), "dlogits: padded class columns")
        return nm.assert_within(dl[:, :ncls], xr["dlogits"], xr["dlogits_bound"], "dlogits", ncls, fam("xent"))
    judge("classifier.dlogits", P3, "dlogits", dlogits)

    def linear_backward(Pj, pname, lin, dz, xin, wj):
        """bias gradient (column sums), weight gradient (the conv weight-gradient kernel over the batch), data gradient"""
        d64, x64 = dz.double(), xin.double()
        Fo, Fi = lin.out_features, lin.in_features
        judge(f"grad:{pname}.bias", Pj, "bias gradient", lambda: nm.assert_sum(
            t(f"grad:{pname}.bias"), d64.sum(0), d64.abs().sum(0), N + 31, f"{Pj}: bias gradient", Fo, fam("linear_bwd")))
        judge(f"grad:{pname}.weight", Pj, "weight gradient", lambda: nm.assert_within(
            t(f"grad:{pname}.weight"), d64.t() @ x64, nm.conv_bound(
                d64.t() @ x64, nm.nominal16(d64, dtype).t() @ nm.nominal16(x64, dtype), N, torch.float32),
            f"{Pj}: weight gradient", Fi, fam("linear_bwd"), (Fo, Fi)))

        def dh():
            ref, mag = d64 @ wj, d64.abs() @ wj.abs()
            return nm.assert_within(t(f"{Pj}.dh"), ref, nm.conv_bound(ref, mag, Fo, dtype), f"{Pj}: dh", Fi,
                                    fam("linear_bwd"), ref.shape)
        judge(f"{Pj}.dh", Pj, "dh", dh)

    linear_backward(P3, f"classifier.{i3}", lin3, dl[:, :ncls], lin_in[i3], w3)
    dh = t(f"{P3}.dh")
    for j, lin, dmod in reversed(hidden):
        Pj = f"classifier.{j}"
        p = float(dmod.p) if dmod is not None else 0.0
        judge(f"{Pj}.dz", Pj, "dz (dropout + ReLU backward)", lambda dh=dh, Pj=Pj, p=p: nm.assert_exact(
            t(f"{Pj}.dz"), pc.fc_act_bwd_ref(dh, t(f"{Pj}.h"), p, dtype), f"{Pj}: dz"))
        linear_backward(Pj, Pj, lin, t(f"{Pj}.dz"), lin_in[j], lin.weight.detach().to(dev).to(dtype).double())
        dh = t(f"{Pj}.dh")
    if drop0 is not None:
        nd = f"classifier.{drop0}.dx"
        p0 = float(model.classifier[drop0].p)
        judge(nd, f"classifier.{drop0}", "feature dropout backward", lambda dh=dh: nm.assert_exact(
            t(nd), pc.fc_act_bwd_ref(dh, t(f"classifier.{drop0}.x"), p0, dtype), nd))
        dh = t(nd)

    # ---------------------------------------------------------------------------------------------- features backward
    def finalize(L, sums, b0, b1, rows, y, coef):
        """dgamma / dbeta / bcoef (BatchNorm) or dbias (bias layer) from the reference sums [C, 2] and their bounds."""
        P, C = L.path, L.conv.out_channels
        if L.bn is None:
            e = b0
            judge(f"grad:{P}.bias", P, "dbias (sum dz)", lambda: nm.assert_within(
                t(f"grad:{P}.bias"), sums[:, 0], e + 2 * U * (sums[:, 0].abs() + e), f"{P}: dbias", C, fam("bwd_finalize")))
            return
        bp = L.bnpath
        count = float(rows * world)
        fr = nm.bn_bwd_finalize_ref(sums[:, 0] * world, sums[:, 1] * world, count, coef, f64(L.bn.weight), 1.0 / world, C)
        judge([f"{P}.bcoef", f"grad:{bp}.weight", f"grad:{bp}.bias"], bp, "dgamma / dbeta / bcoef",
              lambda: nm.check_bwd_finalize_carried(t(f"{P}.bcoef"), t(f"grad:{bp}.weight"), t(f"grad:{bp}.bias"), fr,
                                                    b0 * world, b1 * world, count, 1.0 / world, coef, C, bp,
                                                    fam("bwd_finalize")))
        if L.conv.bias is not None:  # a bias in front of a BatchNorm: the batch mean removes it
            judge(f"grad:{P}.bias", P, "bias gradient (zero in front of a BatchNorm)", lambda: _exact(
                t(f"grad:{P}.bias"), torch.zeros(C, device=dev), f"{P}: bias gradient"))

    def wgrad(L, xin, dy):
        P, conv = L.path, L.conv
        R, S = conv.kernel_size
        st, pd = conv.stride[0], conv.padding[0]

        def run(name, a, b):
            ref, _ = nm.conv_wgrad_ref(xin[a:b], dy[a:b], R, S, st, pd)
            mag = nm.conv_wgrad_nominal_mag(xin[a:b], dy[a:b], R, S, st, pd, dtype)
            got = t(name)
            assert got.shape == (ref.shape[0], ref.shape[3], R, S), f"{name}: gradient shape {tuple(got.shape)}"
            n = (b - a) * dy.shape[1] * dy.shape[2]
            return nm.assert_conv(got.permute(0, 2, 3, 1), ref, mag, n, torch.float32, f"{name}", fam("wgrad"))
        judge(f"grad:{P}.weight", P, "weight gradient", lambda: run(f"grad:{P}.weight", 0, N))
        if f"{P}.wgrad_chunks" in rec.meta:
            for name, (a, b) in chunk_names(P, "wgrad", "wgrad_chunks"):
                judge(name, P, f"weight gradient accumulated over images 0..{b}", lambda name=name, b=b: run(name, 0, b))

    assert layers[-1].pool, "the last feature layer must be pooled (its gradient comes from the classifier)"
    last = layers[-1].path
    hl, wl = t(f"{last}.act").shape[1:3]
    judge(f"{last}.g", last, "g (classifier gradient back in NHWC)", lambda: _exact(
        t(f"{last}.g"), dh.view(N, -1, hl, wl).permute(0, 2, 3, 1), f"{last}: g"))
    for li in range(len(layers) - 1, -1, -1):
        L = layers[li]
        P, conv = L.path, L.conv
        C = conv.out_channels
        y, coef, act, g = t(f"{P}.y"), t(f"{P}.coef"), t(f"{P}.act"), t(f"{P}.g")
        h, w = y.shape[1], y.shape[2]
        rows = N * h * w
        if L.pool:
            k = L.pool
            idx = t(f"{P}.idx")
            ref, mag, carry = pc.pooled_link_ref(y, coef, g, idx, act, k, 0, dtype)
            prow = act.numel() // C
            n_chain = pc.reduce16_plan(prow, C, 2048)[2]
            judge(f"{P}.slots.0", P, "pooled backward sums", lambda ref=ref, mag=mag, carry=carry, n_chain=n_chain, P=P:
                  pc.assert_pooled_link(t(f"{P}.slots.0"), ref, mag, carry, n_chain, f"{P}: pooled sums", fam("pooled_sums")))
            b = torch.stack([(n_chain + 4) * U * mag[:, 0], (n_chain + 8) * U * mag[:, 1]], 1) + carry
            finalize(L, ref, b[:, 0], b[:, 1], rows, y, coef)
            if k == 2:
                d = dict(y=y, dp=g, b=t(f"{P}.bcoef") if L.bn is not None else None)
                dz, dref, dmag = pc.pool2_bwd_ref(d, None, pos=idx, mask=act.double() > 0)
                if L.bn is not None:
                    judge(f"{P}.dy", P, "dy (pool + BatchNorm backward)", lambda dref=dref, dmag=dmag, P=P, C=C: nm.assert_rounded(
                        t(f"{P}.dy"), dref, dmag, dtype, name=f"{P}: dy", C=C, family=fam("pool_bwd")))
                else:
                    judge(f"{P}.dy", P, "dy (pool backward)", lambda dz=dz, P=P: nm.assert_exact(t(f"{P}.dy"), dz, f"{P}: dy"))
            else:
                assert L.bn is None, f"{P}: MaxPool(3, 2) behind a BatchNorm"

                def pool3(y=y, g=g, idx=idx, coef=coef, P=P, C=C, h=h, w=w):
                    rr = cc.stem_tail_ref(dict(y=y, dp=g, idx=idx, coef=coef, b=torch.zeros(3 * C, device=dev)), N, h, w, C, pad=0)
                    share = float(rr["unsure"].double().mean())
                    assert share <= MASK_CAP, f"{P}.dy: {share:.5f} of the pre-activations are too close to zero to call"
                    return pc.assert_pool_bwd(t(f"{P}.dy"), rr, dtype, f"{P}: dy", fam("pool_bwd"))[0]
                judge(f"{P}.dy", P, "dy (pool backward)", pool3)
            dy = t(f"{P}.dy")
        elif L.bn is not None:
            def apply_run(g=g, y=y, P=P, C=C):
                ref, mag = nm.bn_bwd_apply_ref(g.double(), y, t(f"{P}.bcoef"), C)
                return nm.assert_rounded(t(f"{P}.dy").reshape(-1, C), ref, mag, dtype, 8, f"{P}: dy", C, fam("bwd_apply"))
            judge(f"{P}.dy", P, "dy", apply_run)
            dy = t(f"{P}.dy")
        else:
            assert not rec.has(f"{P}.dy"), f"{P}: an unpooled bias layer's conv-output gradient is g itself"
            dy = g
        if li == 0:
            wgrad(L, x_img, dy)
            break
        prev = layers[li - 1]
        PP = prev.path
        xin = t(f"{PP}.act")
        wgrad(L, xin, dy)
        ref, mag = nm.conv_dgrad_ref(dy, sa.krsc(conv, dtype), xin.shape[1], xin.shape[2], 1, conv.padding[0])
        n = C * conv.kernel_size[0] * conv.kernel_size[1]
        if prev.pool:
            judge(f"{PP}.g", P, "data gradient", lambda ref=ref, mag=mag, n=n, PP=PP: nm.assert_conv(
                t(f"{PP}.g"), ref, mag, n, dtype, f"{PP}: g", fam("dgrad")))
            continue
        yp, cp = t(f"{PP}.y"), t(f"{PP}.coef")
        Cp = yp.shape[-1]
        mask, unsure = sa.pre_mask(yp, cp, Cp)
        full = nm.conv_bound(ref, mag, n, dtype)
        dzr, bound = torch.where(mask, ref, zero), torch.where(mask, full, zero)
        judge(f"{PP}.g", P, "data gradient (masked)", lambda dzr=dzr, bound=bound, unsure=unsure, Cp=Cp, PP=PP:
              _masked_compare(t(f"{PP}.g"), dzr, bound, unsure, f"{PP}.g", Cp, fam("dgrad")))
        sb = torch.where(unsure, ref.abs() + full, bound)
        xh = nm.bn_xhat(yp, cp, Cp).view(dzr.shape)
        for name, (a, b) in chunk_names(PP, "slots", "slot_chunks"):
            judge(name, P, f"fused backward sums of images {a}..{b}", lambda name=name, a=a, b=b, dzr=dzr, sb=sb, xh=xh, Cp=Cp:
                  nm.assert_bnb_sums(t(name)[:, 0], t(name)[:, 1], dzr[a:b].reshape(-1, Cp), sb[a:b].reshape(-1, Cp),
                                     xh[a:b].reshape(-1, Cp), name, fam("bnb_sums")))
        prow = yp.numel() // Cp
        d2, s2, x2 = dzr.reshape(-1, Cp), sb.reshape(-1, Cp), xh.reshape(-1, Cp)
        tt = d2 * x2
        b0 = s2.sum(0) + (prow + 4) * U * d2.abs().sum(0)
        b1 = (s2 * x2.abs()).sum(0) + (prow + 4) * U * tt.abs().sum(0)
        finalize(prev, torch.stack([d2.sum(0), tt.sum(0)], 1), b0, b1, prow, yp, cp)
    return sa._finish(wk)
