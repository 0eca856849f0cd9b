"""``convert_convstats`` (ops/convstats.py), the hand-over of a pointwise conv's BatchNorm statistics to the ``BNAct2d``
behind it and the ``--native-convstats`` flag, without a GPU.

* Which conv / BatchNorm pairs the converter forms in the registry models and which it refuses; conversion keeps
  parameters and the state dict, and on the CPU (every module on its fallback path) the results bit for bit.
* The hand-over logic on a stand-in for the native ops (``FakeC`` behind ``native.C``, as tests/test_torch_audit_cpu.py
  installs its emulation): the attribute is consumed once and removed; a stale version, another tensor object or a
  wrong width makes the BatchNorm form its statistics itself.
* The flag parses, and the runner reports ``ignored`` when a prerequisite conversion is off.
"""
import copy
import os
import re
import subprocess
import sys

import pytest
import torch
import torch.nn as nn

from pytorch_distributed_template_amd import cli
from pytorch_distributed_template_amd.models import registry
from pytorch_distributed_template_amd.ops import bnact, native, pointwise
from pytorch_distributed_template_amd.ops.bnact import BNAct2d, CONV_STATS_ATTR, convert_bnact
from pytorch_distributed_template_amd.ops.convstats import convert_convstats
from pytorch_distributed_template_amd.ops.pointwise import PointwiseConv2d, convert_pointwise

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (pointwise convs converted, pairs): every converted 1x1 conv of the MobileNet family, EfficientNet and ShuffleNetV2
# is followed by its BatchNorm inside a Sequential; DenseNet's BatchNorms come BEFORE their convs (pre-activation)
COUNTS = [("mobilenet_v2", 34, 34), ("mobilenet_v3_large", 30, 30), ("mnasnet1_0", 34, 34), ("efficientnet_b0", 32, 32),
          ("shufflenet_v2_x1_0", 10, 10), ("densenet121", 61, 0)]


@pytest.mark.parametrize("arch,n_pw,n_pairs", COUNTS)
def test_convert_counts(arch, n_pw, n_pairs):
    model = registry.create(arch)
    assert convert_convstats(model) == 0  # nothing converted yet
    assert convert_pointwise(model) == n_pw
    assert convert_convstats(model) == 0  # the BatchNorms are still stock modules
    convert_bnact(model)
    assert convert_convstats(model) == n_pairs
    assert sum(m.emit_stats for m in model.modules() if isinstance(m, PointwiseConv2d)) == n_pairs
    assert convert_convstats(model) == 0  # idempotent


def test_bnact_alone_forms_no_pair():
    model = registry.create("mobilenet_v2")
    convert_bnact(model)
    assert convert_convstats(model) == 0


def _pair(K=16, bn_features=None, between=None, seq=nn.Sequential):
    mods = [nn.Conv2d(8, K, 1, bias=False)] + ([between] if between is not None else [])
    mods += [nn.BatchNorm2d(K if bn_features is None else bn_features), nn.ReLU6()]
    model = seq(*mods)
    assert convert_pointwise(model) == 1
    convert_bnact(model)
    return model


class _OwnForward(nn.Sequential):
    def forward(self, x):
        for m in self:
            x = m(x)
        return x


def test_pairs_refused():
    assert convert_convstats(_pair()) == 1
    for hooked, pre in ((0, False), (1, False), (0, True), (1, True)):  # across a forward (pre-)hook on either module
        model = _pair()
        if pre:
            model[hooked].register_forward_pre_hook(lambda m, i: None)
        else:
            model[hooked].register_forward_hook(lambda m, i, o: None)
        assert convert_convstats(model) == 0 and not model[0].emit_stats
    assert convert_convstats(_pair(seq=_OwnForward)) == 0  # a Sequential subclass with its own forward
    model = nn.Sequential(nn.Conv2d(8, 16, 1, bias=False), nn.Conv2d(16, 12, 1, bias=False), nn.BatchNorm2d(12))
    convert_pointwise(model), convert_bnact(model)  # 12 channels: neither the second conv nor the BatchNorm qualifies
    assert convert_convstats(model) == 0
    model = _pair()
    model[1] = BNAct2d(16, momentum=None)  # a BNAct2d that does not qualify
    assert convert_convstats(model) == 0
    assert convert_convstats(_pair(between=nn.Identity())) == 0  # another module between the two
    assert convert_convstats(_pair(K=16, bn_features=24)) == 0  # widths differ
    # the two as attributes of a plain module: no Sequential order to rely on
    holder = nn.Module()
    holder.conv, holder.bn = nn.Conv2d(8, 16, 1, bias=False), nn.BatchNorm2d(16)
    convert_pointwise(holder), convert_bnact(holder)
    assert convert_convstats(holder) == 0


def test_conversion_keeps_state_and_cpu_results():
    torch.manual_seed(0)
    ref = registry.create("mobilenet_v2", dropout=0.0)
    base = copy.deepcopy(ref)
    convert_pointwise(base), convert_bnact(base)
    model = copy.deepcopy(base)
    keys, params = list(model.state_dict()), dict(model.named_parameters())
    names = [n for n, _ in model.named_modules()]
    assert convert_convstats(model) == 34
    assert list(model.state_dict()) == keys == list(ref.state_dict())
    assert [n for n, _ in model.named_modules()] == names
    assert all(p is params[n] for n, p in model.named_parameters()) and len(dict(model.named_parameters())) == len(params)
    # a deep copy keeps the pairs
    assert sum(m.emit_stats for m in copy.deepcopy(model).modules() if isinstance(m, PointwiseConv2d)) == 34
    x = torch.randn(4, 3, 32, 32)
    for a, b in ((model, base), (model, ref)):  # fallback paths: bit for bit the unconverted models
        a.zero_grad(), b.zero_grad()
        ya, yb = a(x), b(x)
        assert torch.equal(ya, yb)
        ya.square().sum().backward()
        yb.square().sum().backward()
        for (n, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
            assert torch.equal(p.grad, q.grad), n
        for (n, u), (_, v) in zip(a.named_buffers(), b.named_buffers()):
            assert torch.equal(u, v), n
        b.load_state_dict(ref.state_dict()), a.load_state_dict(ref.state_dict())  # same running statistics again


# ------------------------------------------------------------------------------------------ hand-over logic
S = 4  # the stand-in's slot count


class FakeC:
    """The forward launchers of the two modules as plain torch, counting calls.  ``pwconv_fwd_stats`` puts the sums in
    slot 0 and zeros elsewhere; ``bnact_stats`` spreads them over two slots, so the tests can tell who filled them."""

    def __init__(self):
        self.calls = []

    def stat_slots(self):
        return S

    def pwconv_fits(self, M, C, K):
        return True

    def pwconv_fwd(self, x, w, y, M, C, K):
        self.calls.append("pwconv_fwd")
        y.copy_((x.float().reshape(M, C) @ w.float().t()).to(y.dtype).reshape(y.shape))

    def _sums(self, y, C):
        y64 = y.double().reshape(-1, C)
        return torch.stack([y64.sum(0), (y64 * y64).sum(0)], 1)

    def pwconv_fwd_stats(self, x, w, y, slots, M, C, K, max_blocks):
        self.pwconv_fwd(x, w, y, M, C, K)
        self.calls[-1] = "pwconv_fwd_stats"
        slots.view(S, K, 2).zero_()
        slots.view(S, K, 2)[0] = self._sums(y, K)
        return [1, 24]

    def bnact_stats(self, x, slots, rows, C):
        self.calls.append("bnact_stats")
        slots.view(S, C, 2).zero_()
        slots.view(S, C, 2)[:2] = self._sums(x, C) / 2
        return [1, 1]

    def bn_finalize_slots(self, slots, count, gamma, beta, eps, momentum, rm, rv, coef, sums, update):
        self.calls.append("bn_finalize_slots:" + ("conv" if bool((slots.view(S, -1)[1] == 0).all()) else "bn"))
        C = gamma.numel()
        tot = slots.view(S, C, 2).sum(0)
        mean = tot[:, 0] / count
        var = (tot[:, 1] / count - mean * mean).clamp_min(0)
        invstd = 1 / torch.sqrt(var + eps)
        scale = gamma.double() * invstd
        coef.copy_(torch.cat([scale, beta.double() - mean * scale, mean, invstd]).float())

    def bnact_fwd(self, x, coef, out, rows, C, act):
        self.calls.append("bnact_fwd")
        u = x.float().reshape(rows, C) * coef[:C] + coef[C:2 * C]
        out.copy_([u, u.relu(), u.clamp(0, 6)][act].to(out.dtype).reshape(out.shape))


@pytest.fixture
def fake(monkeypatch):
    c = FakeC()
    monkeypatch.setattr(native, "C", c)
    return c


def _modules(dtype=torch.bfloat16):
    torch.manual_seed(2)
    model = _pair()
    assert convert_convstats(model) == 1
    x = torch.randn(2, 8, 5, 5).to(dtype).contiguous(memory_format=torch.channels_last)
    return model[0], model[1], x


def test_handover_consumed_once_and_removed(fake):
    conv, bn, x = _modules()
    y = conv._forward_native(x)
    assert fake.calls == ["pwconv_fwd_stats"]
    slots, version = getattr(y, CONV_STATS_ATTR)
    assert version == y._version and slots.numel() == S * 16 * 2
    handed = bnact.take_conv_stats(y)
    assert handed[0] is slots and not hasattr(y, CONV_STATS_ATTR) and bnact.take_conv_stats(y) is None
    out = bn._forward_native(y, handed)
    assert fake.calls == ["pwconv_fwd_stats", "bn_finalize_slots:conv", "bnact_fwd"]  # no bnact_stats
    # the same BatchNorm on the same tensor again, now without the attribute: its own statistics, the same result
    del fake.calls[:]
    bn2 = copy.deepcopy(bn)
    out2 = bn2._forward_native(y, bnact.take_conv_stats(y))
    assert fake.calls == ["bnact_stats", "bn_finalize_slots:bn", "bnact_fwd"]
    assert torch.equal(out, out2)
    assert int(bn.num_batches_tracked) == 1


def test_stale_or_foreign_stats_are_not_used(fake):
    conv, bn, x = _modules()
    # an in-place change between the two (without autograd, which forbids it on a custom Function's view output)
    with torch.no_grad():
        y = conv._forward_native(x)
        y.mul_(2)
    handed = bnact.take_conv_stats(y)
    assert handed is not None and handed[1] != y._version
    del fake.calls[:]
    bn._forward_native(y, handed)
    assert fake.calls == ["bnact_stats", "bn_finalize_slots:bn", "bnact_fwd"]
    # another tensor object (what a hook returning y.clone() gives): nothing is attached to it
    y = conv._forward_native(x)
    z = y.clone()
    assert bnact.take_conv_stats(z) is None and hasattr(y, CONV_STATS_ATTR)
    del fake.calls[:]
    bn._forward_native(z, bnact.take_conv_stats(z))
    assert fake.calls == ["bnact_stats", "bn_finalize_slots:bn", "bnact_fwd"]
    # slots of another width
    y = conv._forward_native(x)
    slots, version = bnact.take_conv_stats(y)
    del fake.calls[:]
    bn._forward_native(y, (slots[:S * 8 * 2], version))
    assert fake.calls == ["bnact_stats", "bn_finalize_slots:bn", "bnact_fwd"]


def test_conv_emits_only_when_paired_and_training(fake):
    conv, bn, x = _modules()
    conv.eval()
    y = conv._forward_native(x)
    assert fake.calls == ["pwconv_fwd"] and not hasattr(y, CONV_STATS_ATTR)
    conv.train()
    conv.emit_stats = False
    y = conv._forward_native(x)
    assert fake.calls == ["pwconv_fwd", "pwconv_fwd"] and not hasattr(y, CONV_STATS_ATTR)
    assert PointwiseConv2d.emit_stats is False and "emit_stats" not in PointwiseConv2d(8, 16, 1, bias=False).__dict__


def test_forward_removes_the_attribute_on_every_path(fake):
    """``BNAct2d.forward`` on its fallback paths (a CPU tensor here; eval mode): the attribute goes, the stock result stays."""
    _, bn, _ = _modules()
    ref = copy.deepcopy(bn)
    for mode in ("train", "eval"):
        getattr(bn, mode)(), getattr(ref, mode)()
        y = torch.randn(2, 16, 5, 5)
        setattr(y, CONV_STATS_ATTR, (torch.zeros(S * 16 * 2, dtype=torch.float64), y._version))
        out = bn(y)
        assert not hasattr(y, CONV_STATS_ATTR)
        assert torch.equal(out, ref(y)) and fake.calls == []


def test_eight_argument_apply_still_works(fake):
    """``_BNActFn.apply`` with its eight arguments (tests/test_torch_audit_cpu.py's call) forms its own statistics."""
    _, bn, x = _modules()
    y = torch.randn(2, 16, 5, 5).bfloat16().contiguous(memory_format=torch.channels_last)
    out = bnact._BNActFn.apply(y, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps, bn.momentum, bn.act)
    assert fake.calls == ["bnact_stats", "bn_finalize_slots:bn", "bnact_fwd"] and out.shape == y.shape


# ------------------------------------------------------------------------------------------ flag and runner
def test_flag_parses():
    for mode in ("dp", "ddp", "ddp_amp"):
        p = cli.build_parser(mode)
        assert p.parse_args([]).native_convstats == "off"
        assert p.parse_args(["--native-convstats", "on"]).native_convstats == "on"
        assert p.parse_args(["--native-convstats", "off"]).native_convstats == "off"
        with pytest.raises(SystemExit):
            p.parse_args(["--native-convstats", "auto"])


def _run(tmp_path, tag, extra):
    out = str(tmp_path / ("out_" + tag))
    args = ["dataparallel.py", "--outpath", out, "-a", "mobilenet_v2", "-b", "4", "--synthetic", "--synthetic-train-size",
            "8", "--synthetic-val-size", "4", "--image-size", "32", "--num-classes", "10", "-j", "0", "--epochs", "1",
            "--iters-per-epoch", "2", "--val-iters", "1", "--exist-policy", "delete", "-p", "1", "--seed", "3",
            "--no-tensorboard"] + list(extra)
    env = dict(os.environ, PYTHONUNBUFFERED="1", OMP_NUM_THREADS="2", HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable] + args, cwd=ROOT, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    log = open(os.path.join(out + "_mobilenet_v2", "experiment.log")).read()
    return log, re.findall(r"Train epoch: \[0/1\]\[\d+/\d+\]\tlr=\S+\tce_loss=(\S+)\ttop1_acc=(\S+)", log)


def test_runner_reports_pairs_or_ignored(tmp_path):
    """Through the runner on the CPU: with both prerequisite conversions the pairs are formed (and the CPU losses are
    those of the run without the flag); with one of them off the flag is reported as ignored and nothing is formed."""
    both = ["--native-pointwise", "on", "--native-bnact", "on"]
    log_on, on = _run(tmp_path, "on", both + ["--native-convstats", "on"])
    log_off, off = _run(tmp_path, "off", both)
    log_ign, ign = _run(tmp_path, "ign", ["--native-pointwise", "on", "--native-convstats", "on"])
    assert "=> native convstats: 34 conv/BatchNorm pair(s) of mobilenet_v2 fused" in log_on
    assert "native convstats" not in log_off
    assert "=> native convstats: ignored, " in log_ign and "pair(s)" not in log_ign
    assert len(off) == 2 and on == off == ign, (on, off, ign)
