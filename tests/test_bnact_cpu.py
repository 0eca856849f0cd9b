"""BatchNorm+activation module conversion, the ``--native-bnact`` flag and the error model of the bnact kernel tests,
without a GPU.

* Which BatchNorms of the registry models qualify and which activations they absorb; conversion keeps parameters,
  buffers, state dict, deepcopy / pickle and the CPU results (every module falls back to the stock ops there).
* A CPU run with the flag on equals one with it off, in dp mode and in ddp_amp mode with ``--sync_batchnorm True`` at
  world size 1.
* The bounds of tests/_bnact_numerics.py can pass and can fail, for every activation: a plain fp32 evaluation of each
  formula stays inside its bound; each assertion rejects a one-ulp error, a dropped row, coefficients shifted by one
  channel and a wrong branch at a breakpoint.
"""
import copy
import io
import os
import pickle
import re
import subprocess
import sys

import pytest
import torch
import torch.nn as nn

import _bnact_numerics as bm
import _numerics as nm
from pytorch_distributed_template_amd import cli
from pytorch_distributed_template_amd.models import registry
from pytorch_distributed_template_amd.ops.bnact import ACTS, BNAct2d, convert_bnact, qualifies

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (BatchNorms converted, activations absorbed): 39 of ShuffleNetV2's 56 BatchNorms have channel counts that are no
# multiple of 8; EfficientNet's activations are SiLU and stay torch modules; ResNet's ReLU is no Sequential sibling;
# ConvNeXt has no BatchNorm
COUNTS = [("mobilenet_v2", 52, 35), ("mobilenet_v3_large", 46, 31), ("mobilenet_v3_small", 34, 23),
          ("mnasnet1_0", 52, 35), ("shufflenet_v2_x1_0", 17, 11), ("densenet121", 121, 4), ("efficientnet_b0", 49, 0),
          ("resnet18", 20, 0), ("convnext_tiny", 0, 0)]


@pytest.mark.parametrize("arch,n_bn,n_abs", COUNTS)
def test_convert_counts(arch, n_bn, n_abs):
    model = registry.create(arch)
    ref = registry.create(arch)
    n_act = sum(type(m) in (nn.ReLU, nn.ReLU6, nn.Hardswish) for m in model.modules())
    assert convert_bnact(model) == (n_bn, n_abs)
    mods = [m for m in model.modules() if isinstance(m, BNAct2d)]
    assert len(mods) == n_bn and sum(m.act != "identity" for m in mods) == n_abs
    assert n_act - sum(type(m) in (nn.ReLU, nn.ReLU6, nn.Hardswish) for m in model.modules()) <= n_abs
    assert convert_bnact(model) == (0, 0)  # idempotent
    # module names (Sequential indices included) and state-dict keys are those of the unconverted model
    assert [n for n, _ in model.named_modules()] == [n for n, _ in ref.named_modules()]
    assert list(model.state_dict()) == list(ref.state_dict())
    if arch == "convnext_tiny":
        assert all(type(a) is type(b) for a, b in zip(model.modules(), ref.modules()))  # untouched


def test_qualifying_predicate():
    assert qualifies(nn.BatchNorm2d(8)) and qualifies(nn.BatchNorm2d(2048)) and qualifies(nn.BatchNorm2d(1280))
    for bad in (nn.BatchNorm2d(58), nn.BatchNorm2d(2056), nn.BatchNorm2d(16, affine=False),
                nn.BatchNorm2d(16, track_running_stats=False), nn.BatchNorm2d(16, momentum=None)):
        assert not qualifies(bad), bad
    # only exact nn.BatchNorm2d instances are swapped (SyncBatchNorm, BatchNorm1d and subclasses stay)
    model = nn.Sequential(nn.BatchNorm1d(16), nn.SyncBatchNorm(16), nn.BatchNorm2d(58), nn.ReLU(), nn.BatchNorm2d(16),
                          nn.SiLU(), nn.BatchNorm2d(16), nn.Hardswish())
    assert convert_bnact(model) == (2, 1)
    assert [type(m).__name__ for m in model] == ["BatchNorm1d", "SyncBatchNorm", "BatchNorm2d", "ReLU", "BNAct2d", "SiLU",
                                                 "BNAct2d", "Identity"]
    assert model[4].act == "identity" and model[6].act == "hardswish"
    with pytest.raises(ValueError):
        BNAct2d(16, act="silu")


_HOOK_CALLS = []


def _record_hook(module, inputs, output):  # module level: the model holding it is pickled below
    _HOOK_CALLS.append(type(module).__name__)


def test_conversion_keeps_state_and_results():
    torch.manual_seed(0)
    model = registry.create("mobilenet_v2", dropout=0.0)
    ref = copy.deepcopy(model)
    before = dict(model.state_dict())
    params = dict(model.named_parameters())
    buffers = dict(model.named_buffers())
    hits = [n for n, m in model.named_modules() if type(m) is nn.BatchNorm2d and qualifies(m)]
    del _HOOK_CALLS[:]
    dict(model.named_modules())[hits[3]].register_forward_hook(_record_hook)
    assert convert_bnact(model) == (52, 35)
    after = model.state_dict()
    assert list(after.keys()) == list(before.keys())  # keys and order
    assert all(after[k] is before[k] or torch.equal(after[k], before[k]) for k in before)
    mods = dict(model.named_modules())
    for n in hits:
        m = mods[n]
        assert type(m) is BNAct2d and m.act in ACTS
        assert m.weight is params[n + ".weight"] and m.bias is params[n + ".bias"]  # the very same Parameter objects
        for b in ("running_mean", "running_var", "num_batches_tracked"):
            assert getattr(m, b) is buffers[n + "." + b]
    assert [n for n, _ in model.named_parameters()] == list(params)
    assert [n for n, _ in model.named_buffers()] == list(buffers)
    # deep copy and pickle round trips keep the class, the activation and the values
    acts = [m.act for m in model.modules() if isinstance(m, BNAct2d)]
    for clone in (copy.deepcopy(model), pickle.load(io.BytesIO(pickle.dumps(model)))):
        assert [m.act for m in clone.modules() if isinstance(m, BNAct2d)] == acts
        assert all(torch.equal(a, b) for a, b in zip(clone.state_dict().values(), after.values()))
    x = torch.randn(4, 3, 32, 32)
    # eval mode
    model.eval(), ref.eval()
    with torch.no_grad():
        assert torch.equal(model(x), ref(x))
    assert _HOOK_CALLS == ["BNAct2d"]  # the hook moved with the module
    # train mode: outputs, the running statistics and the parameter gradients of one backward
    model.train(), ref.train()
    ya, yb = model(x), ref(x)
    assert torch.equal(ya, yb)
    ya.square().sum().backward()
    yb.square().sum().backward()
    for (n, p), (_, q) in zip(model.named_parameters(), ref.named_parameters()):
        assert torch.equal(p.grad, q.grad), n
    for (n, a), (_, b) in zip(model.named_buffers(), ref.named_buffers()):
        assert torch.equal(a, b), n
    # the state dict loads into an unconverted model and back
    ref.load_state_dict(model.state_dict())
    model.load_state_dict(ref.state_dict())


@pytest.mark.parametrize("C", [16, 58])
@pytest.mark.parametrize("act", ACTS)
def test_module_constructor_and_cpu_fallback(act, C):
    torch.manual_seed(1)
    a = BNAct2d(C, eps=1e-3, momentum=0.2, act=act)
    b = nn.BatchNorm2d(C, eps=1e-3, momentum=0.2)
    assert list(a.state_dict()) == list(b.state_dict()) and a.act == act and f"act={act}" in repr(a)
    stock = {"identity": nn.Identity(), "relu": nn.ReLU(), "relu6": nn.ReLU6(), "hardswish": nn.Hardswish()}[act]
    x = torch.randn(3, C, 5, 4) * 3
    x1, x2 = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    ya, yb = a(x1), stock(b(x2))
    assert torch.equal(ya, yb)
    ya.square().sum().backward()
    yb.square().sum().backward()
    assert torch.equal(x1.grad, x2.grad) and torch.equal(a.weight.grad, b.weight.grad)
    assert torch.equal(a.running_var, b.running_var) and int(a.num_batches_tracked) == 1
    # the stock module's error for a wrong channel count
    with pytest.raises(RuntimeError) as ea:
        a(torch.randn(2, 8, 3, 3))
    with pytest.raises(RuntimeError) as eb:
        b(torch.randn(2, 8, 3, 3))
    assert str(ea.value) == str(eb.value)


def test_flag_parses():
    for mode in ("dp", "ddp", "ddp_amp"):
        p = cli.build_parser(mode)
        assert p.parse_args([]).native_bnact == "off"
        assert p.parse_args(["--native-bnact", "on"]).native_bnact == "on"
        assert p.parse_args(["--native-bnact", "off"]).native_bnact == "off"
        with pytest.raises(SystemExit):
            p.parse_args(["--native-bnact", "auto"])


def _losses(tmp_path, script, flag, extra=()):
    out = str(tmp_path / ("out_" + script.split(".")[0] + "_" + flag))
    args = [script, "--outpath", out, "-a", "mobilenet_v2", "-b", "4", "--synthetic", "--synthetic-train-size",
            "8", "--synthetic-val-size", "4", "--image-size", "32", "--num-classes", "10", "-j", "0", "--epochs", "1",
            "--iters-per-epoch", "2", "--val-iters", "1", "--exist-policy", "delete", "-p", "1", "--seed", "3",
            "--no-tensorboard", "--native-bnact", flag] + list(extra)
    env = dict(os.environ, PYTHONUNBUFFERED="1", OMP_NUM_THREADS="2", HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable] + args, cwd=ROOT, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    log = open(os.path.join(out + "_mobilenet_v2", "experiment.log")).read()
    return log, re.findall(r"Train epoch: \[0/1\]\[\d+/\d+\]\tlr=\S+\tce_loss=(\S+)\ttop1_acc=(\S+)", log)


def test_cpu_run_with_flag_on_equals_off(tmp_path):
    """Two iterations of mobilenet_v2 on CPU through the runner: the converted modules fall back to the stock ops, so
    the loss lines are those of the unconverted run."""
    log_on, on = _losses(tmp_path, "dataparallel.py", "on")
    log_off, off = _losses(tmp_path, "dataparallel.py", "off")
    assert len(off) == 2 and on == off, (on, off)
    assert "=> native bnact: 52 BatchNorm(s) of mobilenet_v2 converted, 35 activation(s) fused" in log_on
    assert "native bnact" not in log_off


def test_sync_batchnorm_at_world_one_still_converts(tmp_path):
    """``--sync_batchnorm True`` in ddp_amp mode at world size 1: the trainer converts to SyncBatchNorm only under
    ``sync_bn and dist.is_initialized() and dist.get_world_size() > 1`` (engine/torch_trainer.py), which is false here,
    so the runner's matching condition keeps the flag in force: the BatchNorms are converted, nothing is ignored, and
    the losses are those of the run with the flag off."""
    log_on, on = _losses(tmp_path, "distributed_syncBN_amp.py", "on", ("--sync_batchnorm", "True"))
    log_off, off = _losses(tmp_path, "distributed_syncBN_amp.py", "off", ("--sync_batchnorm", "True"))
    assert len(off) == 2 and on == off, (on, off)
    assert "=> not use sync BN" in log_on
    assert "=> native bnact: 52 BatchNorm(s) of mobilenet_v2 converted, 35 activation(s) fused" in log_on
    assert "native bnact: ignored" not in log_on and "native bnact" not in log_off


# ------------------------------------------------------------------------------------------------ the error model
DTYPES = [torch.bfloat16, torch.float16]


def _case(C, dtype, rows=257, seed=0, tiny=True):
    """x, g (16-bit), coef = [scale | shift | mean | invstd], bcoef = [A | B | Cc]; every coefficient differs per
    channel, u spans all branches of every activation; channel 1 at 1e-6 scale (fp16 subnormal outputs)."""
    g_ = torch.Generator().manual_seed(seed * 1000 + C)
    x = (torch.randn(rows, C, generator=g_) * 2).to(dtype)
    g = torch.randn(rows, C, generator=g_).to(dtype)
    sign = torch.where(torch.rand(C, generator=g_) < 0.3, -1.0, 1.0)
    coef = torch.cat([(torch.rand(C, generator=g_) * 2 + 0.5) * sign, torch.randn(C, generator=g_) * 2,
                      torch.randn(C, generator=g_) * 0.3, torch.rand(C, generator=g_) + 0.5])
    bcoef = torch.cat([(torch.rand(C, generator=g_) + 0.5) * sign, torch.randn(C, generator=g_) * 0.2,
                       torch.randn(C, generator=g_) * 0.1])
    if tiny:
        coef[1] *= 1e-6
        coef[C + 1] *= 1e-6
        for k in range(3):
            bcoef[k * C + 1] *= 1e-6
    return x, g, coef, bcoef


def _branches_hit(u, act):
    bp = bm.BREAKPOINTS[act]
    edges = [-float("inf")] + list(bp) + [float("inf")]
    return all(bool(((u > lo) & (u < hi)).any()) for lo, hi in zip(edges[:-1], edges[1:]))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [8, 24, 1280])
@pytest.mark.parametrize("act", ACTS)
def test_fp32_emulation_of_bnact_fwd_stays_within_the_bound(act, C, dtype):
    x, _, coef, _ = _case(C, dtype)
    u = bm.u_emul(x, coef, C)
    assert _branches_hit(u.double(), act)
    out = bm.act_emul(u, act).to(dtype)
    worst = bm.assert_fwd(out, x, coef, C, act, dtype, name=f"bnact_fwd emulation {act}")
    assert 0.5 < worst <= 1.0  # the half-ulp term is tight
    # also with u rounded twice (a product and a sum instead of the fused multiply-add)
    out2 = bm.act_emul(x.float() * coef[:C] + coef[C:2 * C], act).to(dtype)
    bm.assert_fwd(out2, x, coef, C, act, dtype, name=f"bnact_fwd unfused emulation {act}")
    if dtype == torch.float16:
        assert bool((out[:, 1].float().abs() < 2.0 ** -14).any())  # subnormal outputs were exercised


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("act", ACTS)
def test_fp32_emulation_of_bnact_bwd_apply_stays_within_the_bound(act, dtype):
    C = 96
    x, g, coef, bcoef = _case(C, dtype, seed=3)
    dz = bm.dz_emul(g, bm.u_emul(x, coef, C), act)
    dx = bm.bwd_apply_emul(dz, x, bcoef, C).to(dtype)
    worst = bm.assert_bwd_apply(dx, g, x, coef, bcoef, C, act, dtype, name=f"bnact_bwd_apply emulation {act}")
    assert 0.5 < worst <= 1.0
    # the emulation and the reference took the same branch everywhere: no reference u in the band of a breakpoint
    u, mag_u = bm.u_ref(x, coef, C)
    assert int(bm.near_breakpoint(u, mag_u, act).sum()) == 0


def _chain_sums(dz, x, coef, C, blocks, lanes):
    """The kernel's structure: row r goes to chain (r // lanes % blocks, r % lanes); fp32 chains, an fp32 sum over the
    lanes of a block, fp64 over the blocks."""
    rows = dz.shape[0]
    xh = (x.float().reshape(-1, C) - coef[2 * C:3 * C]) * coef[3 * C:4 * C]
    pad = (-rows) % (blocks * lanes)
    got = []
    for terms in (dz, dz * xh):
        t = torch.cat([terms, torch.zeros(pad, C)]).view(-1, blocks, lanes, C)
        chain = torch.zeros(blocks, lanes, C)
        for i in range(t.shape[0]):
            chain = chain + t[i]
        blk = torch.zeros(blocks, C)
        for r in range(lanes):
            blk = blk + chain[:, r]
        got.append(blk.double().sum(0))
    return torch.stack(got, 1)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("act", ACTS)
def test_fp32_emulation_of_the_bnact_reduce_chain_stays_within_the_bound(act, dtype):
    rows, C, blocks, lanes = 3000, 96, 12, 21
    x, g, coef, _ = _case(C, dtype, rows=rows, seed=5, tiny=False)
    dz = bm.dz_emul(g, bm.u_emul(x, coef, C), act)
    got = _chain_sums(dz, x, coef, C, blocks, lanes)
    worst = bm.assert_bwd_sums(got, g, x, coef, C, act, bm.n_chain(rows, blocks, lanes), name=f"reduce emulation {act}")
    assert worst < 0.5  # rounding errors average out: far below the worst-case chain bound


@pytest.mark.parametrize("dtype", DTYPES)
def test_fp32_emulation_of_the_statistics_chain_stays_within_the_bound(dtype):
    """sum x and sum x^2 (the square of a 16-bit value is exact in fp32): the sum bound on sum|x| and sum x^2."""
    rows, C, blocks, lanes = 3000, 96, 12, 21
    x, _, _, _ = _case(C, dtype, rows=rows, seed=6)
    xf = x.float()
    pad = (-rows) % (blocks * lanes)
    x64 = x.double()
    for terms, ref, mag in ((xf, x64.sum(0), x64.abs().sum(0)), (xf * xf, (x64 * x64).sum(0), (x64 * x64).sum(0))):
        t = torch.cat([terms, torch.zeros(pad, C)]).view(-1, blocks, lanes, C)
        chain = torch.zeros(blocks, lanes, C)
        for i in range(t.shape[0]):
            chain = chain + t[i]
        blk = torch.zeros(blocks, C)
        for r in range(lanes):
            blk = blk + chain[:, r]
        assert nm.assert_sum(blk.double().sum(0), ref, mag, bm.n_chain(rows, blocks, lanes), "stats emulation", C) < 0.5
        with pytest.raises(AssertionError, match="out of bound"):  # one row missing
            nm.assert_sum(ref - terms[-1].double(), ref, mag, bm.n_chain(rows, blocks, lanes), "stats", C)


def _one_ulp_off(out, ref, dtype):
    """``out`` with one ordinary element moved to the neighbouring representable value away from the reference."""
    frac = torch.frexp(ref.abs().float())[0]
    i = int(((frac > 0.5) & (frac < 0.6) & (ref.abs() > 0.1)).flatten().nonzero()[0])
    bad = out.clone().flatten()
    bits = bad.view(torch.int16)
    up = float((bits[i:i + 1] + 1).view(dtype).double().item())
    down = float((bits[i:i + 1] - 1).view(dtype).double().item())
    r = float(ref.flatten()[i].item())
    bits[i] += 1 if abs(up - r) > abs(down - r) else -1
    return bad.view_as(out), i


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("act", ACTS)
def test_elementwise_assertions_reject_one_ulp_and_shifted_coefficients(act, dtype):
    C = 64
    x, g, coef, bcoef = _case(C, dtype, tiny=False)
    u = bm.u_emul(x, coef, C)
    # forward
    out = bm.act_emul(u, act).to(dtype)
    bm.assert_fwd(out, x, coef, C, act, dtype)
    bad, i = _one_ulp_off(out, bm.fwd_ref(x, coef, C, act)[2], dtype)
    with pytest.raises(AssertionError, match=f"worst element {i}, channel {i % C}"):
        bm.assert_fwd(bad, x, coef, C, act, dtype)
    shifted = torch.cat([coef[:C].roll(1), coef[C:2 * C].roll(1), coef[2 * C:]])
    with pytest.raises(AssertionError, match="out of bound"):
        bm.assert_fwd(bm.act_emul(bm.u_emul(x, shifted, C), act).to(dtype), x, coef, C, act, dtype)
    # backward apply
    dz = bm.dz_emul(g, u, act)
    dx = bm.bwd_apply_emul(dz, x, bcoef, C).to(dtype)
    bm.assert_bwd_apply(dx, g, x, coef, bcoef, C, act, dtype)
    bad, i = _one_ulp_off(dx, bm.bwd_apply_ref(g, x, coef, bcoef, C, act)[0], dtype)
    with pytest.raises(AssertionError, match=f"worst element {i}, channel {i % C}"):
        bm.assert_bwd_apply(bad, g, x, coef, bcoef, C, act, dtype)
    with pytest.raises(AssertionError, match="out of bound"):  # [A | B | Cc] of the neighbouring channel
        bm.assert_bwd_apply(bm.bwd_apply_emul(dz, x, bcoef.view(3, C).roll(1, 1).reshape(-1), C).to(dtype), g, x, coef,
                            bcoef, C, act, dtype)
    if act != "identity":  # scale / shift of the neighbouring channel: another u, another branch or slope
        with pytest.raises(AssertionError, match="out of bound"):
            bm.assert_bwd_apply(bm.bwd_apply_emul(bm.dz_emul(g, bm.u_emul(x, shifted, C), act), x, bcoef, C).to(dtype), g,
                                x, coef, bcoef, C, act, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("act", ACTS)
def test_sum_assertion_rejects_a_missing_row_and_shifted_coefficients(act, dtype):
    rows, C, blocks, lanes = 3000, 96, 12, 21
    chain = bm.n_chain(rows, blocks, lanes)
    x, g, coef, _ = _case(C, dtype, rows=rows, seed=5, tiny=False)
    ref, _ = bm.bwd_reduce_ref(g, x, coef, C, act)
    bm.assert_bwd_sums(ref, g, x, coef, C, act, chain)
    short, _ = bm.bwd_reduce_ref(g[:-1], x[:-1], coef, C, act)
    for k in (0, 1):  # each of the two sums on its own
        got = ref.clone()
        got[:, k] = short[:, k]
        with pytest.raises(AssertionError, match="out of bound"):
            bm.assert_bwd_sums(got, g, x, coef, C, act, chain)
    rolled, _ = bm.bwd_reduce_ref(g, x, coef.view(4, C).roll(1, 1).reshape(-1), C, act)
    with pytest.raises(AssertionError, match="out of bound"):
        bm.assert_bwd_sums(rolled, g, x, coef, C, act, chain)


# (u at or next to a breakpoint, the derivative torch defines there, the wrong branch's)
WRONG_BRANCH = {"relu": [(0.0, 0.0, 1.0)], "relu6": [(0.0, 0.0, 1.0), (6.0, 0.0, 1.0)],
                "hardswish": [(-3.0, 0.0, -0.5), (3.0, 1.0, 1.5)]}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("act", ["relu", "relu6", "hardswish"])
def test_assertions_reject_a_wrong_branch_at_a_breakpoint(act, dtype):
    """scale = 1, shift = 0, x exactly on the breakpoint: the reference derivative is torch's, and the other branch's
    derivative fails the backward-apply and the sum assertions.  The activations themselves are continuous, so for the
    forward assertion the wrong branch is taken a quarter beside the breakpoint."""
    C, rows = 8, 64
    coef = torch.cat([torch.ones(C), torch.zeros(C), torch.zeros(C), torch.ones(C)])
    bcoef = torch.cat([torch.ones(C), torch.zeros(C), torch.zeros(C)])
    g = (torch.rand(rows, C, generator=torch.Generator().manual_seed(1)) + 0.5).to(dtype)
    for bp, right, wrong in WRONG_BRANCH[act]:
        x = torch.full((rows, C), bp).to(dtype)
        u, _ = bm.u_ref(x, coef, C)
        assert torch.equal(bm.dact_ref(u, act), torch.full_like(u, right))
        x_ag = x.double().requires_grad_(True)  # torch's own convention at the breakpoint
        {"relu": torch.relu, "relu6": nn.functional.relu6, "hardswish": nn.functional.hardswish}[act](x_ag).sum().backward()
        assert torch.equal(x_ag.grad, torch.full_like(u, right))
        ok = bm.dz_emul(g, bm.u_emul(x, coef, C), act)
        assert torch.equal(ok, g.float() * right)
        bm.assert_bwd_apply(ok.to(dtype), g, x, coef, bcoef, C, act, dtype)
        bad = g.float() * wrong
        with pytest.raises(AssertionError, match="out of bound"):
            bm.assert_bwd_apply(bad.to(dtype), g, x, coef, bcoef, C, act, dtype)
        # xhat = x here: the second sum is bp * the first (zero at bp = 0, where only the first can tell)
        good = torch.stack([ok.double().sum(0), (ok.double() * bp).sum(0)], 1)
        bm.assert_bwd_sums(good, g, x, coef, C, act, bm.n_chain(rows, 1, 32))
        with pytest.raises(AssertionError, match="out of bound"):
            bm.assert_bwd_sums(torch.stack([bad.double().sum(0), (bad.double() * bp).sum(0)], 1), g, x, coef, C, act,
                               bm.n_chain(rows, 1, 32))
        # forward, a quarter beside the breakpoint, evaluated on the other side's branch
        for side in (-0.25, 0.25):
            xs = torch.full((rows, C), bp + side).to(dtype)
            us = bm.u_emul(xs, coef, C)
            bm.assert_fwd(bm.act_emul(us, act).to(dtype), xs, coef, C, act, dtype)
            # (the formula of the branch above the breakpoint, of the branch below it)
            other = {"relu": {0.0: (us, torch.zeros_like(us))},
                     "relu6": {0.0: (us, torch.zeros_like(us)), 6.0: (torch.full_like(us, 6.0), us)},
                     "hardswish": {-3.0: (us * (us + 3) / 6, torch.zeros_like(us)),
                                   3.0: (us, us * (us + 3) / 6)}}[act][bp][0 if side < 0 else 1]
            with pytest.raises(AssertionError, match="out of bound"):
                bm.assert_fwd(other.to(dtype), xs, coef, C, act, dtype)
