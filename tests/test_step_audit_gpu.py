"""Teacher-forced audit of ResNetExecutor steps on the MI355X: every intermediate of a training step (and of an eval step)
per element against fp64, layer by layer (tests/_step_audit.py), through the recording proxy of tests/_tape.py.

Two input geometries:

* ``small``: N = 3, 3 x 64 x 64.  Layer4 runs at 2 x 2: its BatchNorm count is 12, so a count that is one image off or a
  biased running variance is a large error.
* ``strip``: N = 2, 3 x 32 x 224.  The stem gives 16 x 112 and layer1 runs at 8 x 56, so the width-56 routes of the
  224 x 224 step are eligible at a seventh of its cost.  H = 32 is enough for every name of R18_224_KERNELS and of
  R50_224_KERNELS (tests/test_executor_gpu.py) but one, asserted through ``dispatch_counts()``: ``conv_pp_512x128`` is
  the shipped tile table's choice for ResNet-50's 1x1 convs at the 224 x 224 shapes (keyed by N, H, W), which no strip
  has; that route stays with test_train_step_matches_reference_224.

The executor is built with PDT_WGRAD_STREAM=0: one stream, so the proxy's clone after a plain synchronize holds what the
kernel wrote (test_side_stream_bitwise_equals_single_stream proves the two schedules equal bit for bit).
"""
import pytest
import torch

import _step_audit as sa
from _tape import Tape
from test_executor_gpu import R18_224_KERNELS, R50_224_KERNELS

pytestmark = pytest.mark.gpu
DEV = "cuda"
GEOM = {"small": (3, 64, 64), "strip": (2, 32, 224)}
DT = {"bf16": torch.bfloat16, "fp16": torch.float16}

# the specialised routes the strip must dispatch (module docstring)
STRIP_R18 = R18_224_KERNELS
STRIP_R50 = tuple(k for k in R50_224_KERNELS if k != "conv_pp_512x128")


class _Rig:
    """A model, its executor behind a Tape, and the audit of one step at a time."""

    def __init__(self, arch, dtype, monkeypatch, geom, ex_kw=None, seed=0):
        from pytorch_distributed_template_amd.models import resnet
        from pytorch_distributed_template_amd.models.executor import ResNetExecutor
        from pytorch_distributed_template_amd.optim.flat import FlatBuffers, FlatParams
        monkeypatch.setenv("PDT_WGRAD_STREAM", "0")
        torch.manual_seed(seed)
        model = getattr(resnet, arch)()
        k = 0
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.data.uniform_(0.5, 1.5)
                m.bias.data.uniform_(-0.2, 0.2)
                m.running_mean.uniform_(-0.5, 0.5)
                m.running_var.uniform_(0.5, 1.5)
                # every BatchNorm its own eps and momentum: a finalize that takes them from another layer shows.  The
                # momenta are within 0.3 % of 1: the running statistics then ARE the last batch's, and the eval step of
                # a random-init bottleneck network stays inside the fp16 range (a blend with the initial buffers or with
                # the statistics from before the SGD step leaves activations of 1e4 .. 1e8 in fp32 torch)
                m.eps = (1e-5, 1e-4, 1e-3)[k % 3]
                m.momentum = (1.0, 0.999, 0.998, 0.997)[k % 4]
                k += 1
        self.model, self.dtype, self.arch = model, dtype, arch
        self.flat = FlatParams(model, DEV, dtype)
        FlatBuffers(model, DEV)
        self.ex = ResNetExecutor(model, self.flat, DEV, dtype, **(ex_kw or {}))
        assert self.ex.side is None
        self.tape = Tape(self.ex.C)
        self.ex.C = self.tape
        self.saved = None
        fwd = self.ex._forward

        def keep(images, train):
            self.saved = fwd(images, train)
            return self.saved
        self.ex._forward = keep
        self.N, self.H, self.W = GEOM[geom]
        self.family = f"step/{arch}/{'bf16' if dtype == torch.bfloat16 else 'fp16'}/{geom}"
        self.seed = seed

    def batch(self, k, u8=False):
        g = torch.Generator(device=DEV).manual_seed(1000 * self.seed + k)
        shape = (self.N, 3, self.H, self.W)
        x = torch.randint(0, 256, shape, generator=g, device=DEV, dtype=torch.uint8) if u8 else \
            torch.randn(shape, generator=g, device=DEV)
        return x, torch.randint(0, 1000, (self.N,), generator=g, device=DEV)

    def run(self, x, t, train=True, loss_scale=None, grad_div=None, world=None):
        """Run one step and audit it; returns (record, findings)."""
        self.tape.clear()
        before = {n: b.clone() for n, b in self.model.named_buffers()}
        if train:
            logits, met = self.ex.train_step(x, t, loss_scale=loss_scale, grad_div=grad_div)
        else:
            logits, met = self.ex.eval_step(x, t)
        torch.cuda.synchronize()
        rec = sa.extract_record(self.ex, self.saved, self.tape, self.model, train)
        assert torch.equal(rec.t["logits"], logits) and torch.equal(rec.t["met"], met)
        found = sa.audit(rec, self.model, before, x, t, self.dtype, train,
                         None if loss_scale is None else float(loss_scale), grad_div, world, family=self.family)
        return rec, found

    def step(self, x, t, train=True, loss_scale=None, grad_div=None, world=None, what="step"):
        """``run`` with nothing found and everything judged; returns the record."""
        rec, found = self.run(x, t, train, loss_scale, grad_div, world)
        assert not found, f"{self.family} {what}: {len(found)} findings\n" + sa.report(found)
        # completeness: every parameter gradient, every buffer, every recorded tensor judged, every ratio <= 1
        if train:
            for n, _ in self.model.named_parameters():
                assert f"grad:{n}" in rec.judged, n
        for n, _ in self.model.named_buffers():
            assert f"buf:{n}" in rec.judged, n
        assert set(rec.t) <= set(rec.judged) and max(rec.judged.values()) <= 1.0
        return rec


def _counts():
    from pytorch_distributed_template_amd.ops import native
    return {k: v for k, v in native.C.dispatch_counts().items() if v}


@pytest.mark.parametrize("geom,arch", [("small", "resnet18"), ("small", "resnet50"), ("small", "resnext50_32x4d"),
                                       ("strip", "resnet18"), ("strip", "resnet50")])
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_two_training_steps_and_an_eval_step(arch, dt, geom, monkeypatch):
    """Step 1; FusedSGD (lr 0.1, momentum 0.9, wd 1e-4) + update_derived; step 2 on another batch, judged with the
    UPDATED master parameters rounded to the 16-bit type (a stale shadow, derived layout or coefficient shows per
    element); then an eval step on a third batch.  The strip asserts its specialised routes."""
    from pytorch_distributed_template_amd.ops import native
    from pytorch_distributed_template_amd.optim.sgd import FusedSGD
    rig = _Rig(arch, DT[dt], monkeypatch, geom)
    native.C.reset_dispatch_counts()
    rig.step(*rig.batch(1), what="step 1")
    if geom == "strip":
        counts = _counts()
        print("dispatch", arch, geom, counts)
        missing = [k for k in (STRIP_R18 if arch == "resnet18" else STRIP_R50) if not counts.get(k)]
        assert not missing, (missing, counts)
    before = rig.flat.data.clone()
    FusedSGD(rig.flat, lr=0.1, momentum=0.9, weight_decay=1e-4).step()
    rig.ex.update_derived()
    torch.cuda.synchronize()
    assert not torch.equal(before, rig.flat.data), "the optimizer step changed nothing"
    rig.step(*rig.batch(2), what="step 2")
    rig.step(*rig.batch(3), train=False, what="eval")


def test_a_skipped_update_derived_is_found_where_the_stale_layouts_are_read(monkeypatch):
    """Negative control on the device: step 1, FusedSGD, NO update_derived, step 2.  The derived buffer then holds the
    previous step's stem, fc and backward-data layouts while every other forward conv reads the fresh shadow: the audit
    must report the stem's y, the fc logits and dfeat, every conv's data gradient and the BatchNorm sums fused into
    them -- and, judged from the recorded inputs, nothing else."""
    from pytorch_distributed_template_amd.optim.sgd import FusedSGD
    rig = _Rig("resnet18", torch.bfloat16, monkeypatch, "small", seed=5)
    rig.step(*rig.batch(1), what="step 1")
    FusedSGD(rig.flat, lr=0.1, momentum=0.9, weight_decay=1e-4).step()
    torch.cuda.synchronize()
    rig.family = "step_negative_control"  # its ratios are failures by design: kept out of the step/... records
    _, found = rig.run(*rig.batch(2))
    got = {(f.path, f.quantity) for f in found}
    assert {("conv1", "y"), ("fc", "logits (padded, no bias)"), ("fc", "dfeat")} <= got, sorted(got)
    convs = [f"{p}.conv{i}" for p, b in sa.block_paths(rig.model) for i in range(1, len(sa.block_convs(b)) + 1)]
    missing = [c for c in convs if not any(p == c and q.startswith("data gradient") for p, q in got)]
    assert not missing, (missing, sorted(got))
    stray = [(p, q) for p, q in got if not (p in ("conv1", "fc") or q.startswith("data gradient")
                                            or q == "dgamma / dbeta / bcoef")]
    assert not stray, stray


SWITCHES = ["compact_ds", "fuse_block_bn_maxhw", "fuse_pre", "fuse_pre_1x1", "stem_fused", "bwd_buf_per_block",
            "wgrad_l1", "stem_kernel"]


def _pre_launches(tape):
    n3 = tape.count("conv_fwd_pre")
    n1 = sum(1 for c in tape.named("conv1x1_c64") if c.kwargs.get("pre") is not None)
    return n3, n1


@pytest.mark.parametrize("arch,dt,geom", [("resnet18", "bf16", "strip"), ("resnet50", "fp16", "small")])
@pytest.mark.parametrize("switch", SWITCHES)
def test_executor_switch_takes_the_alternative_route_and_passes(switch, arch, dt, geom, monkeypatch):
    """One executor switch off at a time: the audit passes on the alternative route, and the tape / the dispatch counters
    show that the alternative ran."""
    from pytorch_distributed_template_amd.ops import native
    rig = _Rig(arch, DT[dt], monkeypatch, geom, seed=1)
    ex, tape = rig.ex, rig.tape
    setattr(ex, switch, 0 if switch == "fuse_block_bn_maxhw" else False)
    native.C.reset_dispatch_counts()
    rec = rig.step(*rig.batch(1), what=f"{switch} off")
    counts = _counts()
    nblocks = len(ex.blocks)
    ds_blocks = [p for p, b in sa.block_paths(rig.model) if b.downsample is not None]
    if switch == "compact_ds":
        assert not counts.get("conv_dgrad_compact_residual"), counts
        assert not any(rec.meta[f"{p}.downsample.0.dx_compact"] for p in ds_blocks)
        assert all(c.args[23] < 0 for c in tape.named("conv_dgrad_bn"))
    elif switch == "fuse_block_bn_maxhw":
        assert tape.count("bn_bwd_reduce") == nblocks
        assert not any(rec.meta[f"{p}.gin_is_dz"] for p, _ in sa.block_paths(rig.model))
        ident = [p for p, b in sa.block_paths(rig.model) if b.downsample is None]
        assert ident and all(rec.has(f"{p}.dz") for p in ident)  # dz_id written by the separate apply
    elif switch == "fuse_pre":
        assert _pre_launches(tape) == (0, 0)
        assert not any(v for k, v in rec.meta.items() if k.endswith("fused_into_consumer"))
    elif switch == "fuse_pre_1x1":
        assert _pre_launches(tape)[1] == 0
        assert not counts.get("conv1x1_c64_fused_bn_relu"), counts
    elif switch == "stem_fused":
        assert tape.count("stem_pool_bwd_apply") == 1 and tape.count("conv_wgrad_stem_fused") == 0
        assert rec.has("conv1.dy") and not counts.get("wgrad_stem_fused"), counts
    elif switch == "bwd_buf_per_block":
        keys = [k[0] for k in ex._bufs]
        assert "dy_a" in keys and not any(isinstance(k, tuple) and k[0] == "dy_a" for k in keys)
    elif switch == "wgrad_l1":
        assert tape.count("conv_wgrad_3x3c64") == 0 and tape.count("conv_fwd_pre") == 0
        assert not counts.get("wgrad3x3_c64"), counts
    elif switch == "stem_kernel":
        assert tape.count("stem_fwd") == 0 and not counts.get("stem_fwd"), counts
        assert any(c.args[29] == 4 for c in tape.named("conv_fwd"))  # the generic kernel in window mode (cs = 4)


def test_default_routes_of_the_switch_cases(monkeypatch):
    """The routes the switch cases turn off are the ones the default executor takes at those geometries (so each switch
    case really changes the step)."""
    from pytorch_distributed_template_amd.ops import native
    for arch, dt, geom in (("resnet18", "bf16", "strip"), ("resnet50", "fp16", "small")):
        rig = _Rig(arch, DT[dt], monkeypatch, geom, seed=1)
        native.C.reset_dispatch_counts()
        rec = rig.step(*rig.batch(1), what="default")
        tape = rig.tape
        assert tape.count("bn_bwd_reduce") == 1 and tape.count("stem_fwd") == 1
        assert tape.count("conv_wgrad_stem_fused") == 1 and not rec.has("conv1.dy")
        assert any(v for k, v in rec.meta.items() if k.endswith("dx_compact")) == (arch == "resnet18")
        n3, n1 = _pre_launches(tape)
        assert (n3 > 0 and tape.count("conv_wgrad_3x3c64") > 0) if arch == "resnet18" else n1 > 0, (n3, n1)


def test_uint8_images_are_normalised_in_the_pack(monkeypatch):
    """uint8 input: the pack is judged against (x / 255 - mean) / std per element, the rest of the step follows."""
    rig = _Rig("resnet18", torch.bfloat16, monkeypatch, "small", seed=2)
    x, t = rig.batch(1, u8=True)
    rig.step(x, t, what="uint8")
    assert rig.tape.count("stem_pack_u8") == 1 and rig.tape.count("stem_pack") == 0


def test_loss_scale_and_grad_div(monkeypatch):
    """fp16 with loss_scale = 1024 and grad_div = 2N: every gradient carries 1024 / 2N, loss and metrics are unscaled
    (the audit's references are built with that factor from dlogits on)."""
    rig = _Rig("resnet18", torch.float16, monkeypatch, "small", seed=3)
    x, t = rig.batch(1)
    rec = rig.step(x, t, loss_scale=torch.tensor(1024.0, device=DEV), grad_div=2 * rig.N, what="loss scale")
    plain = _Rig("resnet18", torch.float16, monkeypatch, "small", seed=3)
    rec0 = plain.step(x, t, what="no loss scale")
    assert torch.equal(rec.t["met"], rec0.t["met"]) and torch.equal(rec.t["logits"], rec0.t["logits"])
    ratio = rec.t["grad:fc.bias"].double().abs().sum() / rec0.t["grad:fc.bias"].double().abs().sum()
    assert abs(float(ratio) - 512.0) < 1.0, float(ratio)


@pytest.mark.parametrize("arch", ["resnet18", "resnet50"])
@pytest.mark.parametrize("world", [1, 2])
def test_syncbn_arithmetic_on_one_gpu(arch, world, monkeypatch):
    """The SyncBN finalize path without processes: world 1 with an identity all-reduce, world 2 simulated by doubling
    the sums (two ranks with identical batches: the count doubles, the statistics stay, dgamma / dbeta are the local
    share).  A downsample block's two forward statistics share ONE all-reduce: bn_slot_sum twice, then the reduce."""
    calls = []
    rig = None

    def allreduce(t):
        calls.append(len(rig.tape.calls))
        if world == 2:
            t.mul_(2)
    rig = _Rig(arch, torch.bfloat16, monkeypatch, "small", seed=4,
               ex_kw=dict(syncbn_allreduce=allreduce, syncbn_world=world))
    assert rig.ex.syncbn and rig.ex.syncbn_world == world
    rig.step(*rig.batch(1), world=world, what=f"syncbn world {world}")
    tc = rig.tape.calls
    paired = [n for n in calls if n >= 2 and tc[n - 1].name == "bn_slot_sum" and tc[n - 2].name == "bn_slot_sum"]
    nds = sum(1 for _, b in sa.block_paths(rig.model) if b.downsample is not None)
    assert len(paired) == nds, (len(paired), nds)
    assert rig.tape.count("bn_finalize_slots") == 0 and rig.tape.count("bn_bwd_finalize_slots") == 0
    nbn = sum(1 for m in rig.model.modules() if isinstance(m, torch.nn.BatchNorm2d))
    assert rig.tape.count("bn_finalize") == nbn and rig.tape.count("bn_bwd_finalize") == nbn
