"""The optimiser, AMP-state and weight-layout kernels called directly: sgd, nonfinite_check, amp_update /
DeviceGradScaler, cast16, gather16, scatter32.

sgd runs three steps against an fp64 recurrence with the bound 6u * sum_steps(|p| + lr*|buf|) per element
(tests/_numerics.py sgd_ref, u = 2**-24); everything else here is exact: flags, scales and trackers, casts (bitwise
equal to torch's round-to-nearest-even ``.to(dtype)``) and index moves.  Sizes above 8192 * 256 elements make the
grid-stride loops of these kernels run a second pass.

Worst observed error / bound on an MI355X with these seeds (information, not a threshold): sgd 0.23 of its bound;
every other check in this file is exact.
"""
import pytest
import torch

import _numerics as nm

pytestmark = pytest.mark.gpu

DEV = "cuda"
GRID = 8192 * 256  # elements of one pass of the optimiser kernels' grid

def _C():
    from pytorch_distributed_template_amd.ops import native
    return native.C


SGD_CASES = {
    "wd_mask_bf16_shadow": dict(wd_mask=True, loss_scale=None, gscale=0.5, momentum=0.9, shadow=torch.bfloat16),
    "loss_scale_fp16_shadow": dict(wd_mask=False, loss_scale=1024.0, gscale=0.125, momentum=0.9, shadow=torch.float16),
    "zero_momentum_no_shadow": dict(wd_mask=True, loss_scale=None, gscale=1.0, momentum=0.0, shadow=None),
    "found_inf_zero_runs": dict(wd_mask=False, loss_scale=1024.0, gscale=0.125, momentum=0.9, shadow=None, found=0.0),
}


@pytest.mark.parametrize("case", list(SGD_CASES))
def test_sgd_three_steps_against_fp64(case):
    """d = g*gs + wd*p*mask; buf = d (first step) | momentum*buf + d; p -= lr*buf; shadow = p rounded to 16 bits.
    n = 8192*256 + 777 runs the second grid pass.  With momentum 0 the momentum buffer (NaN here) is neither read nor
    written.  loss_scale = 1024 with gscale = 1/8 folds to gs = 2**-13 exactly."""
    cfg = SGD_CASES[case]
    torch.manual_seed(11)
    n = GRID + 777
    lr, wd, mom = 0.1, 1e-4, cfg["momentum"]
    p = torch.randn(n, device=DEV)
    ls = cfg["loss_scale"]
    g = torch.randn(n, device=DEV) * (ls or 1.0)
    wdm = (torch.rand(n, device=DEV) < 0.5).float() if cfg["wd_mask"] else None
    buf = torch.full((n,), float("nan"), device=DEV)
    sh = torch.full((n,), float("nan"), dtype=cfg["shadow"], device=DEV) if cfg["shadow"] else None
    lst = torch.full((1,), ls, device=DEV) if ls else None
    found = torch.full((1,), cfg["found"], device=DEV) if "found" in cfg else None
    ref_p, ref_b, bound = nm.sgd_ref(p, g, torch.zeros(n, device=DEV), wdm, lr, mom, wd, cfg["gscale"] / (ls or 1.0), 3)
    for step in range(3):
        _C().sgd(p, g, buf, sh, wdm, lr, mom, wd, cfg["gscale"], lst, found, step == 0)
    nm.assert_within(p, ref_p, bound, f"sgd {case}: p", family="2 sgd")
    if mom != 0.0:
        # lr * buf is one of the terms of p's bound: the same bound over lr holds buf
        nm.assert_within(buf, ref_b, bound / lr, f"sgd {case}: buf", family="2 sgd")
    else:
        assert bool(torch.isnan(buf).all()), "momentum 0 must leave the momentum buffer untouched"
    if sh is not None:
        assert torch.equal(sh.view(torch.int16), p.to(cfg["shadow"]).view(torch.int16))


@pytest.mark.parametrize("shadow", [torch.bfloat16, torch.float16, None])
def test_sgd_found_inf_skips_the_whole_step(shadow):
    torch.manual_seed(12)
    n = GRID + 777
    p, g, buf = torch.randn(n, device=DEV), torch.randn(n, device=DEV), torch.randn(n, device=DEV)
    sh = torch.randn(n, device=DEV).to(shadow) if shadow else None
    p0, b0 = p.clone(), buf.clone()
    s0 = sh.clone() if shadow else None
    found = torch.ones(1, device=DEV)
    _C().sgd(p, g, buf, sh, None, 0.1, 0.9, 1e-4, 1.0, None, found, False)
    assert torch.equal(p.view(torch.int32), p0.view(torch.int32))
    assert torch.equal(buf.view(torch.int32), b0.view(torch.int32))
    if shadow:
        assert torch.equal(sh.view(torch.int16), s0.view(torch.int16))


def test_nonfinite_check_positions_and_values():
    """NaN, +inf and -inf set the flag wherever they sit (first element, inside the first wave's range, the last
    element, the second grid pass); the largest finite magnitudes and subnormals do not; a set flag stays set."""
    torch.manual_seed(13)
    n = GRID + 100
    g = torch.randn(n, device=DEV)
    found = torch.zeros(1, device=DEV)
    _C().nonfinite_check(g, found)
    assert found.item() == 0.0
    for pos in (0, 100, n - 1, GRID + 5):
        for bad in (float("nan"), float("inf"), float("-inf")):
            keep = g[pos].item()
            g[pos] = bad
            found.zero_()
            _C().nonfinite_check(g, found)
            assert found.item() == 1.0, f"{bad} at {pos} not detected"
            g[pos] = keep
    for pos, v in ((0, 3e38), (100, -3e38), (n - 1, 1e-40), (GRID + 5, -1e-45)):
        g[pos] = v
    found.zero_()
    _C().nonfinite_check(g, found)
    assert found.item() == 0.0
    found.fill_(1.0)
    _C().nonfinite_check(g, found)
    assert found.item() == 1.0


def _expected_scaler(scale, tracker, flag, growth, backoff, interval):
    """torch.amp.GradScaler's update rule (_amp_update_scale_) in fp32."""
    s = torch.tensor(scale, dtype=torch.float32)
    if flag:
        return float(s * torch.tensor(backoff, dtype=torch.float32)), 0
    tracker += 1
    if tracker == interval:
        grown = s * torch.tensor(growth, dtype=torch.float32)
        return (float(grown) if bool(torch.isfinite(grown)) else float(s)), 0
    return float(s), tracker


@pytest.mark.parametrize("growth,backoff,init", [(2.0, 0.5, 2.0 ** 16), (1.7, 0.3, 1000.0), (2.0, 0.5, 3e38)])
def test_device_grad_scaler_follows_grad_scaler_semantics(growth, backoff, init):
    """A scripted overflow sequence with growth_interval = 3: after every update the device scaler (amp_update kernel)
    equals the CPU path of the same class and the upstream rule exactly; with scale = 3e38 a growth would overflow fp32:
    the scale is kept and the tracker reset."""
    from pytorch_distributed_template_amd.amp.scaler import DeviceGradScaler
    dev = DeviceGradScaler(DEV, init_scale=init, growth_factor=growth, backoff_factor=backoff, growth_interval=3)
    cpu = DeviceGradScaler("cpu", init_scale=init, growth_factor=growth, backoff_factor=backoff, growth_interval=3)
    scale, tracker = float(torch.tensor(init, dtype=torch.float32)), 0
    for step, flag in enumerate([0, 0, 0, 1, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 1, 0]):
        for s in (dev, cpu):
            s.found_inf.fill_(float(flag))
            s.update()
        scale, tracker = _expected_scaler(scale, tracker, flag, growth, backoff, 3)
        assert dev.get_scale() == cpu.get_scale() == scale, f"step {step}: {dev.get_scale()} {cpu.get_scale()} {scale}"
        assert int(dev._tracker.item()) == int(cpu._tracker.item()) == tracker, f"step {step}: tracker"
        assert dev.found_inf.item() == float(flag)  # update only reads the flag; unscale_check clears it
    if init == 3e38:
        assert dev.get_scale() <= float(torch.tensor(3e38, dtype=torch.float32))


def test_amp_update_kernel_direct_and_unscale_check():
    scale = torch.full((1,), 4.0, device=DEV)
    tracker = torch.full((1,), 1, dtype=torch.int32, device=DEV)
    found = torch.zeros(1, device=DEV)
    _C().amp_update(scale, tracker, found, 2.0, 0.5, 2)
    assert scale.item() == 8.0 and tracker.item() == 0 and found.item() == 0.0
    found.fill_(1.0)
    _C().amp_update(scale, tracker, found, 2.0, 0.5, 2)
    assert scale.item() == 4.0 and tracker.item() == 0 and found.item() == 1.0
    from pytorch_distributed_template_amd.amp.scaler import DeviceGradScaler
    s = DeviceGradScaler(DEV)
    g = torch.ones(1000, device=DEV)
    s.found_inf.fill_(1.0)
    s.unscale_check(g)
    assert s.found_inf.item() == 0.0  # cleared, then left clear by a finite gradient
    g[999] = float("nan")
    s.unscale_check(g)
    assert s.found_inf.item() == 1.0


@pytest.mark.parametrize("device", ["cuda", "cpu"])
def test_device_grad_scaler_state_dict_round_trip(device):
    from pytorch_distributed_template_amd.amp.scaler import DeviceGradScaler
    a = DeviceGradScaler(device, init_scale=1024.0, growth_interval=5)
    for flag in (0, 0, 1, 0, 0):
        a.found_inf.fill_(float(flag))
        a.update()
    sd = a.state_dict()
    assert sd["scale"] == 512.0 and sd["_growth_tracker"] == 2 and sd["growth_interval"] == 5
    b = DeviceGradScaler(device)
    b.load_state_dict(sd)
    assert b.state_dict() == sd
    assert torch.equal(b._scale, a._scale) and torch.equal(b._tracker, a._tracker)
    off = DeviceGradScaler(device, enabled=False)
    assert off.state_dict() == {} and off.get_scale() == 1.0 and off.scale_tensor is None
    off.update()


def _cast_inputs(dtype):
    torch.manual_seed(14)
    n = GRID + 4099
    x = torch.randn(n, device=DEV) * torch.exp(torch.randn(n, device=DEV) * 4)
    mant = 8 if dtype == torch.bfloat16 else 11  # significand bits
    h = 2.0 ** -mant  # half an ulp at 1
    special = [0.0, -0.0, 1 + h, 1 + 3 * h, -(1 + h), -(1 + 3 * h), 1 + h + 2.0 ** -23, 1 + h - 2.0 ** -24, 2 + 2 * h,
               70000.0, -70000.0, 65504.0, 65519.996, 65520.0, -65520.0, 3.4e38, -3.4e38,
               2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -25 * (1 + 2.0 ** -10), 5 * 2.0 ** -26, 1e-8, -1e-8, 6e-8,
               2.0 ** -14, 2.0 ** -14 * (1 - 2.0 ** -11), 2.0 ** -14 * (1 - 2.0 ** -12),
               1e-38, 1e-39, -1e-39, 1e-40, 9.2e-41, 4.6e-41, 1e-45, float("inf"), float("-inf")]
    sp = torch.tensor(special, dtype=torch.float32, device=DEV)
    x[:sp.numel()] = sp
    x[GRID + 7:GRID + 7 + sp.numel()] = sp  # and in the second grid pass
    return x, sp.numel()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_cast16_is_round_to_nearest_even_everywhere(dtype):
    """cast16 == x.to(dtype) bitwise over random values across the exponent range, exact rounding ties, +-0, fp16
    overflow (70000 -> inf, 65520 -> inf), subnormals of the target and of fp32, +-inf; NaN stays NaN."""
    x, nsp = _cast_inputs(dtype)
    nan_at = [nsp + 3, GRID + 4000]
    for i in nan_at:
        x[i] = float("nan")
    out = torch.full((x.numel(),), 1.0, dtype=dtype, device=DEV)
    _C().cast16(x, out)
    ref = x.cpu().to(dtype)
    got = out.cpu()
    isn = torch.isnan(ref.float())
    assert int(isn.sum()) == len(nan_at) and torch.equal(torch.isnan(got.float()), isn)
    gb, rb = got.view(torch.int16)[~isn], ref.view(torch.int16)[~isn]
    bad = (gb != rb).nonzero().flatten()
    assert bad.numel() == 0, (f"{bad.numel()} elements differ from round-to-nearest-even; first: x = "
                              f"{x.cpu()[~isn][bad[0]].item()!r} -> {got[~isn][bad[0]].item()!r}, expected "
                              f"{ref[~isn][bad[0]].item()!r}")
    if dtype == torch.float16:
        assert got[9].item() == float("inf") and got[10].item() == float("-inf")  # 70000, -70000


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_gather16(dtype):
    """dst[i] = src[idx[i]], 0 for a negative index; bitwise, second grid pass included."""
    torch.manual_seed(15)
    ns, nd = 100003, GRID + 33
    src = torch.randn(ns, device=DEV).to(dtype)
    idx = torch.randint(-3, ns, (nd,), device=DEV, dtype=torch.int32)
    idx[0], idx[1], idx[nd - 1] = -1, ns - 1, 0
    dst = torch.full((nd,), float("nan"), dtype=dtype, device=DEV)
    _C().gather16(src, idx, dst)
    ref = torch.where(idx >= 0, src[idx.clamp_min(0).long()], torch.zeros((), dtype=dtype, device=DEV))
    assert bool((idx < 0).any())
    assert torch.equal(dst.view(torch.int16), ref.view(torch.int16))


def test_scatter32():
    """dst[idx[i]] = src[i] over distinct indices; destinations not addressed keep their sentinel."""
    torch.manual_seed(16)
    n, extra = GRID + 33, 50
    src = torch.randn(n, device=DEV)
    perm = torch.randperm(n + extra, device=DEV)
    idx = perm[:n].to(torch.int32)
    dst = torch.full((n + extra,), -7.5, device=DEV)
    _C().scatter32(src, idx, dst)
    ref = torch.full((n + extra,), -7.5, device=DEV)
    ref[idx.long()] = src
    assert torch.equal(dst.view(torch.int32), ref.view(torch.int32))
    assert bool((dst[perm[n:]] == -7.5).all())
