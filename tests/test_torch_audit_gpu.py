"""Teacher-forced audit of torch-engine training steps with all four native conversions on the MI355X
(tests/_torch_audit.py through the recording proxy of tests/_tape.py): every launch of every converted module of
MobileNetV2 and MobileNetV3-small per element against fp64 from the operands that launch read, and the binding of
every module to its weights, gradients and buffers bit for bit.  tests/test_torch_audit_cpu.py proves the audit itself.

Rig: ``registry.create(arch, dropout=0.0)``, ``convert_stem`` / ``convert_pointwise`` / ``convert_depthwise`` /
``convert_bnact``; every BatchNorm re-initialised as tests/test_step_audit_gpu.py does (weight U(0.5, 1.5), bias
U(-0.2, 0.2), random running statistics, its own eps and momentum: a zero shift would put every element of a dead
channel on a breakpoint); ``TorchTrainer(model, "cuda", dtype=dt)`` without AMP; two training steps on different batches,
each audited (the second against the UPDATED masters: a stale 16-bit operand shows).

Geometries: ``square`` N = 8, 3 x 64 x 64 (the size of every MobileNetV2 step test; the last stages run at 2 x 2: 32
rows per channel) and ``odd`` N = 6, 3 x 48 x 40 (maps 24 x 20, 12 x 10, 6 x 5, 3 x 3, 2 x 2: stride-2 depthwise on odd
maps, ragged M everywhere, 24 rows at the end).  The fp16 arms are unscaled on purpose: their gradients are partly
subnormal, which the MFMA weight gradients are judged for over the nominal magnitudes (tests/_numerics.py).

No tolerance is tuned; the worst error / bound ratios are in profiles/torch_audit_ratios.md.
"""
import time

import pytest
import torch

import _torch_audit as ta
from _tape import Tape

pytestmark = pytest.mark.gpu
DEV = "cuda"
GEOM = {"square": (8, 64, 64), "odd": (6, 48, 40)}
DT = {"bf16": torch.bfloat16, "fp16": torch.float16}
# converted modules (stem, pointwise, depthwise, (BatchNorms, activations absorbed)): tests/test_*_cpu.py assert the same
COUNTS = {"mobilenet_v2": (1, 34, 17, (52, 35)), "mobilenet_v3_small": (1, 22, 11, (34, 23))}
# what must have run natively: the activations and the (kernel, stride) pairs of the depthwise convs
ACTS = {"mobilenet_v2": {"relu6", "identity"}, "mobilenet_v3_small": {"hardswish", "relu", "identity"}}
DW = {"mobilenet_v2": {(3, 1), (3, 2)}, "mobilenet_v3_small": {(3, 1), (3, 2), (5, 1), (5, 2)}}
assert set().union(*ACTS.values()) == {"identity", "relu", "relu6", "hardswish"}


class _Rig:
    def __init__(self, arch, dt, geom, monkeypatch, seed=0):
        from pytorch_distributed_template_amd.engine.torch_trainer import TorchTrainer
        from pytorch_distributed_template_amd.models import registry
        from pytorch_distributed_template_amd.ops import bnact, depthwise, native, pointwise, stemconv
        torch.manual_seed(seed)
        model = registry.create(arch, dropout=0.0)
        self.counts = (stemconv.convert_stem(model), pointwise.convert_pointwise(model),
                       depthwise.convert_depthwise(model), bnact.convert_bnact(model))
        k = 0
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.data.uniform_(0.5, 1.5)
                m.bias.data.uniform_(-0.2, 0.2)
                m.running_mean.uniform_(-0.5, 0.5)
                m.running_var.uniform_(0.5, 1.5)
                # every BatchNorm its own eps and momentum: a finalize that takes them from another layer shows
                m.eps = (1e-5, 1e-4, 1e-3)[k % 3]
                m.momentum = (0.1, 0.01, 0.2, 0.05)[k % 4]
                k += 1
        self.arch, self.dtype, self.model = arch, DT[dt], model
        self.N, self.H, self.W = GEOM[geom]
        self.seed = seed
        self.family = f"torch_audit/{arch}/{dt}/{geom}"
        self.hooks = ta.Hooks(model)
        self.tr = TorchTrainer(model, DEV, dtype=self.dtype)
        assert self.tr.scaler.scale_tensor is None  # no loss scaling: the fp16 gradients are what the kernels get
        self.tape = Tape(native.C)
        monkeypatch.setattr(native, "C", self.tape)

    def batch(self, k):
        g = torch.Generator(device=DEV).manual_seed(1000 * self.seed + k)
        x = torch.randn((self.N, 3, self.H, self.W), generator=g, device=DEV)
        return x, torch.randint(0, 1000, (self.N,), generator=g, device=DEV)

    def run(self, k):
        """One recorded training step and its audit: (findings, judged)."""
        self.tape.clear()
        self.hooks.clear()
        p0, b0 = ta.snapshot(self.model)
        logits, met = self.tr.train_step(*self.batch(k))
        torch.cuda.synchronize()
        assert bool(torch.isfinite(logits).all()) and bool(torch.isfinite(met).all())
        return ta.audit(self.tape, self.model, self.hooks.io, p0, b0, self.dtype, self.tr.flat, family=self.family)

    def step(self, k):
        found, judged = self.run(k)
        assert not found, f"{self.family} step {k}: {len(found)} findings\n" + ta.report(found)
        # completeness: every launch, every parameter gradient and buffer of a converted module judged, every ratio <= 1
        assert all(f"call:{c.index}" in judged for c in self.tape.calls if c.name not in ta.OUT_OF_SCOPE)
        for path, m in ta.converted(self.model):
            for n, _ in m.named_parameters(recurse=False):
                assert f"grad:{path}.{n}" in judged, (path, n)
            for n, _ in m.named_buffers(recurse=False):
                assert f"buf:{path}.{n}" in judged, (path, n)
        assert max(judged.values()) <= 1.0
        return judged


def _launch_counts(arch):
    n_st, n_pw, n_dw, (n_bn, _) = COUNTS[arch]
    want = {"stem3x3_fwd": n_st, "stem3x3_wgrad": n_st, "wgrad_reduce": n_st + n_pw + n_dw,
            "bn_finalize_slots": n_bn, "bn_slot_sum": n_bn, "bn_bwd_finalize": n_bn, "sgd": 1}
    want.update({k: n_pw for k in ("pwconv_fwd", "pwconv_dgrad", "pwconv_wgrad")})
    want.update({k: n_dw for k in ("dwconv_fwd", "dwconv_dgrad", "dwconv_wgrad")})
    want.update({k: n_bn for k in ("bnact_stats", "bnact_fwd", "bnact_bwd_reduce", "bnact_bwd_apply")})
    return want


@pytest.mark.parametrize("geom", ["square", "odd"])
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("arch", ["mobilenet_v2", "mobilenet_v3_small"])
def test_two_training_steps_of_the_converted_network(arch, dt, geom, monkeypatch):
    """Step 1; the trainer's own FusedSGD update; step 2 on another batch, judged against the updated masters.  Every
    converted module launches each of its kernels exactly once per step (no module falls back at these geometries), and
    the dispatch counters agree with the tape."""
    from pytorch_distributed_template_amd.ops import bnact
    t0 = time.perf_counter()
    rig = _Rig(arch, dt, geom, monkeypatch)
    assert rig.counts == COUNTS[arch]
    rig.tape.reset_dispatch_counts()
    for k in (1, 2):
        before = rig.tr.flat.data.clone()
        rig.step(k)
        assert not torch.equal(before, rig.tr.flat.data), "the optimizer step changed nothing"
        got = {}
        for c in rig.tape.calls:
            got[c.name] = got.get(c.name, 0) + 1
        assert got == _launch_counts(arch), got
        assert {bnact.ACTS[c.args[5]] for c in rig.tape.named("bnact_fwd")} == ACTS[arch]
        for name in ("dwconv_fwd", "dwconv_dgrad", "dwconv_wgrad"):
            assert {(c.args[7], c.args[8]) for c in rig.tape.named(name)} == DW[arch], name
    counts = rig.tape.dispatch_counts()
    for name in ("pwconv_fwd", "dwconv_dgrad", "bnact_bwd_apply", "stem3x3_wgrad"):
        assert counts.get(name, 0) == 2 * _launch_counts(arch)[name], (name, counts.get(name))
    if dt == "fp16":  # how much of the unscaled fp16 gradients is subnormal (what the nominal magnitudes are for)
        dys = [rig.tape.value_at(c.index, c.args[1]) for c in rig.tape.named("pwconv_wgrad")]
        sub = sum(int(((d != 0) & (d.float().abs() < 2.0 ** -14)).sum()) for d in dys)
        print(f"{rig.family}: {sub} of {sum(d.numel() for d in dys)} dY elements of the pointwise weight gradients are "
              "subnormal")
    print(f"{rig.family}: {time.perf_counter() - t0:.1f} s")
